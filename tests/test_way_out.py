"""The order in which the editors' output leaves the device (csrc/host/way_out.h: the copies home through the two pinned
pieces, the encoder's batches in two buffers with two pairs of size words, the release of the caller's output slots), run on
the CPU: tools/way_out_check.cc plugs a memcpy and a toy encoder into the same template gpu_out.h plugs HIP into, and is built
with AddressSanitizer and UBSan.  What it asserts at every call, its shapes and the failures it injects: its header comment.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sanitizer_build(tmp_path):
    """the check program built with ASan + UBSan, or the reason why this compiler cannot"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler: the library's host side needs one"
    base = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the compiler can: the program then does not care what else the process loads
    for flags in (base + ["-static-libasan", "-static-libubsan"], base):
        p = subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
        if p.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        return None, "%s has no sanitizer runtime here: %s" % (cxx, p.stderr.strip()[-200:])
    exe = tmp_path / "way_out_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "way_out_check.cc")], check=True)
    return str(exe), None


def test_the_order_of_the_way_out_under_the_sanitizers(tmp_path):
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    p = subprocess.run([exe], capture_output=True, text=True)  # (a program of its own: the sanitizers' runtimes are linked into it)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    runs, _, rest = p.stdout.partition(" runs, ")
    assert int(runs) >= 200 and int(rest.split()[0]) > 10000 and "every byte and every order agreed" in p.stdout, p.stdout
