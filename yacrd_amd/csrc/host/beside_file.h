// beside_file.h — an output file that appears in its place whole or not at all: written as `out_path.XXXXXX` beside it,
// renamed over it by commit(), unlinked by the destructor when commit() was not reached.  Plain C++ (checked by
// tools/segment_pump_check.cc).  What may be replaced at all is the caller's rule, looked at before open().
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

namespace yseg {

struct BesideFile {
    int fd = -1;
    std::string tmp, path;
    BesideFile() = default;
    BesideFile(const BesideFile &) = delete;
    BesideFile &operator=(const BesideFile &) = delete;
    // mode: `existing`'s when the file replaces one whose mode is to be kept, else what open(2) would give a new file
    bool open(const char *out_path, const struct stat *existing = nullptr)
    {
        path = out_path;
        tmp = path + ".XXXXXX";
        fd = mkstemp(&tmp[0]);
        if (fd < 0) {
            tmp.clear();
            return false;
        }
        if (existing) (void)fchmod(fd, existing->st_mode & 07777);
        else {
            const mode_t um = umask(0);
            umask(um);
            (void)fchmod(fd, 0666 & ~um);
        }
        return true;
    }
    // every byte is in: close, move into place; false (and nothing left behind): one of the two failed
    bool commit()
    {
        const int f = fd;
        fd = -1;
        const bool ok = f >= 0 && ::close(f) == 0 && ::rename(tmp.c_str(), path.c_str()) == 0;
        if (ok) tmp.clear();
        else drop();
        return ok;
    }
    void drop()
    {
        if (fd >= 0) (void)::close(fd);
        fd = -1;
        if (!tmp.empty()) (void)::unlink(tmp.c_str());
        tmp.clear();
    }
    ~BesideFile() { drop(); }
};

} // namespace yseg
