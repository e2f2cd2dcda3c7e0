/*
 * yacrd_engine.h — C ABI of the MI355X bad-region engine (libyacrd_hip.so).
 *
 * This is the drop-in boundary for natir/yacrd's `trait BadPart` (reference src/stack.rs:35-41):
 * a Rust `struct FromGpu: BadPart` calls yacrd_engine_run() from
 * `compute_all_bad_part` (src/stack.rs:143-162, called once from src/main.rs:78) and answers
 * `get_bad_part` (src/stack.rs:164-169) / `get_reads` (:171-173) from the returned CSR.
 *
 * Data contract (CSR over reads, the device-side replacement of
 * `MapReads2Ovl = FxHashMap<String,(Vec<(u32,u32)>,usize)>`, src/reads2ovl/mod.rs:41):
 *   offsets   u64[R+1]  prefix sums of intervals per read (offsets[0] = 0)
 *   intervals u32[2*I]  (start,end) pairs in any order within a read (src/io.rs:23-34 cols
 *                       3-4 / 8-9; both sides of each overlap line, src/reads2ovl/mod.rs:108-109)
 *   lengths   u32[R]    first length seen per read (src/reads2ovl/fullmemory.rs:82-90)
 * Results:
 *   bad_offsets u64[R+1], bad_regions u32[2*G] (begin,end) pairs in the reference's order
 *   (src/stack.rs:61-139), read_type u8[R] (src/editor/mod.rs:85-100).
 *
 * Conventions: every function returns 0 on success or a YACRD_E* code; the message for the
 * last error on the calling thread is yacrd_last_error().  Calls on one engine must not
 * overlap; different engines (one per GPU) may be driven from different threads/processes.
 * Plain C types only — no torch, no HIP types in the signatures.
 *
 * Deviations from the reference, all loud: read lengths must fit u32 (the reference keeps
 * usize and truncates with `as u32` when emitting, src/stack.rs:112); `coverage` is u32 (the
 * CLI's u64, src/cli.rs:53-54, saturates — a read never has 2^32 intervals here either).
 */
#ifndef YACRD_ENGINE_H
#define YACRD_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YACRD_ABI_VERSION 7 /* (yacrd_engine_ingest_report[_mem], yacrd_engine_write_report[_mem] and yacrd_engine_edit_fastq[_mem, _gzip_mem, _gzip_file] are additive: found by the symbol, like the editors) 7: yacrd_timing.predicted / prediction_misses / build_switches / sorting_build; 6: yacrd_engines_ingest_overlaps[_mem]; 5: YACRD_F_ONE_LAUNCH, yacrd_timing.one_launch; 4: yacrd_timing.screen_items, yacrd_engine_ingest_overlaps_mem */

/* src/editor/mod.rs:42-59 ReadType; numeric encoding is ours, names are the reference's. */
enum { YACRD_NOT_BAD = 0, YACRD_CHIMERIC = 1, YACRD_NOT_COVERED = 2 };

enum {
    YACRD_OK = 0,
    YACRD_EINVAL = 1,  /* bad argument / malformed CSR */
    YACRD_ENODEV = 2,  /* no usable gfx950 device, or HIP runtime error */
    YACRD_ENOMEM = 3,  /* host or device allocation failed */
    YACRD_EINTERNAL = 4,
    YACRD_EFALLBACK = 5 /* yacrd_engine_ingest_paf: the input is not for the device parser; use the host parser */
};

typedef struct yacrd_engine yacrd_engine;

typedef struct {
    int32_t device_id;  /* HIP device ordinal; -1 = the calling thread's current device */
    uint32_t flags;     /* YACRD_F_* */
} yacrd_engine_cfg;

#define YACRD_F_DEFAULT 0u
/* record HIP events around every phase and every class kernel (costs ~3 us of stream time per
 * event); by default only the dominant class kernel is timed */
#define YACRD_F_TIMING_FULL 32u
/* record no HIP events at all (yacrd_timing stays 0): what a caller that only wants results uses */
#define YACRD_F_NO_TIMING 1024u
/* the run's final wait polls an event and sleeps in between instead of spinning in
 * hipStreamSynchronize: for several engines per CPU core (pipelined batches, many GPUs).
 * Engines created on the same device pipeline their batches (yacrd_engine_submit / _collect from
 * one host thread, or one host thread each). */
#define YACRD_F_BLOCKING_WAIT 2048u
/* the dominant kernel carries its start / stop events on every 8th run of the engine only (counted
 * from its creation or the last yacrd_engine_timing_total(reset), whose next run is a timed one): attached
 * events cost ~10 us per batch (host + stream) against a 20 us kernel; yacrd_timing.timed_runs says how
 * many runs were timed */
#define YACRD_F_TIMING_SAMPLED 32768u
/* Latency over throughput, for callers that run ONE short batch at a time (the CLI once its input is in HBM): a batch of
 * fewer than 400 000 reads whose reads all have at most 256 intervals runs as one kernel launch — no size-class plan, no
 * class counts, no prediction, one dispatch instead of three (csrc/one_batch.h: 100 000 reads in 51-55 us instead of 64-66).
 * Any other batch takes the default path, as does a batch in which that launch met a read it does not handle (found on
 * the device; the batch is then run again).  Callers that keep several batches in flight are better off without. */
#define YACRD_F_ONE_LAUNCH 4194304u
/* (the A/B and test switches that pin a kernel family or a build live in yacrd_engine_debug.h; the
 * product path is flags = 0) */

/* Host-side result, allocated by the engine, released with yacrd_result_free(). */
typedef struct {
    uint64_t n_reads;
    uint64_t n_regions;    /* G */
    uint64_t *bad_offsets; /* R+1 */
    uint32_t *bad_regions; /* 2*G */
    uint8_t *read_type;    /* R */
} yacrd_result;

/* Device-side result: pointers into engine-owned HBM, valid until the next run / destroy. */
typedef struct {
    uint64_t n_reads;
    uint64_t n_regions;
    const void *d_bad_offsets; /* u64[R+1] */
    const void *d_bad_regions; /* u32[2*G] */
    const void *d_read_type;   /* u8[R]   */
} yacrd_device_result;

/* Wall times of the last run, measured with HIP events on the engine's stream.  An event costs
 * ~3 us of stream time, so by default only the dominant kernel is timed (class_ms of the class
 * with the most intervals, or fused_ms — the latter with start / stop events attached to the
 * launch, i.e. the dispatch's own timestamps); plan_ms, sweep_*_ms, compact_ms, total_ms and class_ms
 * of the other classes need YACRD_F_TIMING_FULL and are 0 without it. */
typedef struct {
    float h2d_ms;
    float plan_ms;          /* size-class binning */
    float sweep_small_ms;   /* one read per wavefront (dominant kernel) */
    float sweep_medium_ms;  /* one read per workgroup, LDS resident */
    float sweep_general_ms; /* global-memory path: huge / degenerate reads */
    float compact_ms;       /* scan + compact + classify */
    float d2h_ms;
    float total_ms;         /* first kernel start -> last kernel end */
    uint64_t n_small, n_medium, n_general;     /* reads per class */
    uint64_t iv_small, iv_medium, iv_general;  /* intervals per class */
    /* per size class (YACRD_CLASS_NAMES order): own kernel time, reads, intervals */
    float class_ms[12];
    uint64_t class_reads[12];
    uint64_t class_intervals[12];
    /* the classes R2..H16 run as ONE launch (sweep_small_fused_kernel): its time and what it
     * processed; class_ms of those classes is then 0 */
    float fused_ms;
    uint64_t fused_reads, fused_intervals;
    /* reads whose events were thinned by the coverage pre-filter before the sort (counted only
     * under YACRD_F_COUNT_PREFILTERED) */
    uint64_t prefiltered_reads;
    /* reads (and their intervals) the fused kernel's screen could not finish and left to the follow-on
     * kernel's sort (they are part of fused_reads / fused_intervals: the screen loads and bins them);
     * screened: 1 when the run's fused launch was the screening build (the count of such runs in
     * yacrd_engine_timing_total) */
    uint64_t deferred_reads;
    uint64_t deferred_intervals;
    uint32_t screened;
    /* runs in which the dominant kernel carried its start / stop events: 1 or 0 for one run, the count
     * in yacrd_engine_timing_total (fused_ms / class_ms are sums over these runs: with
     * YACRD_F_TIMING_SAMPLED not every run is one) */
    uint32_t timed_runs;
    /* groups of list entries per wavefront the screen ran with (1 or 2; the last run's): 2 for long launches unless the one
     * before left more than a tenth of its reads to the sort — then the one-item build with the sliding windows runs */
    uint32_t screen_items;
    /* 1: the screen ran in the build with the second looks (sliding windows; always one item); the count of such runs in
     * yacrd_engine_timing_total */
    uint32_t screen_wide;
    /* 1: the batch ran as ONE launch (YACRD_F_ONE_LAUNCH and every read within 256 intervals); the count of such runs in
     * yacrd_engine_timing_total */
    uint32_t one_launch;
    /* 1: the batch was run a second time with the workgroup classes down the three-launch chain, because a workgroup of the
     * persistent screen + fallback kernel ran out of looks at its queue slot (its grid was not resident as a whole: a device
     * shared with another process, a CU mask); the count of such runs in yacrd_engine_timing_total.  (Was reserved0: ABI 5.) */
    uint32_t fused_reruns;
    /* Which path a run took — what makes a short batch's latency depend on the engine's history (ABI 7; all four: 0 / 1 for
     * one run, the count of such runs in yacrd_engine_timing_total):
     * predicted: the sweeps were launched without waiting for the plan's class counts, their grids sized from the engine's
     *   previous run of the same shape;
     * prediction_misses: the run's prediction did not hold at the final sync (a class beyond its grid, a read for the
     *   device-wide or the exact path, a region overflow) and the batch was run again down the synchronous path;
     * build_switches: the register classes' launch took another build than the engine's previous run (sorting / screening,
     *   one item / two items / second looks: see screen_items, screen_wide);
     * sorting_build: that launch was the sorting build (the screen switched off by size or by the last batches' deferral rate). */
    uint32_t predicted;
    uint32_t prediction_misses;
    uint32_t build_switches;
    uint32_t sorting_build;
} yacrd_timing;

/* size classes, in the order of yacrd_timing.class_*: R<K> = four reads per wavefront (16-lane
 * rows, K keys per lane), H16 = two per wavefront, W<K> = one per wavefront, M1/M2 = one per
 * workgroup (LDS), BIG = device-wide path (> 16384 intervals) */
#define YACRD_CLASS_NAMES "R2,R4,R8,R16,H16,W2,W4,W8,W16,M1,M2,BIG"

int yacrd_abi_version(void);
const char *yacrd_last_error(void);

int yacrd_engine_create(const yacrd_engine_cfg *cfg, yacrd_engine **out);
void yacrd_engine_destroy(yacrd_engine *e);

/* Blocking: H2D, kernels, D2H.  Replaces FromOverlap::compute_all_bad_part
 * (src/stack.rs:143-162) + the per-read type_of_read of the report loop
 * (src/main.rs:80-84, src/editor/mod.rs:71). */
int yacrd_engine_run(yacrd_engine *e, const uint64_t *offsets, const uint32_t *intervals,
                     const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                     double not_coverage, yacrd_result *out);
void yacrd_result_free(yacrd_result *r);

/* Same computation on inputs already resident in HBM (device pointers, same layout).
 * n_intervals must equal offsets[n_reads].  Blocking (synchronises the engine's stream). */
int yacrd_engine_run_device(yacrd_engine *e, const void *d_offsets, const void *d_intervals,
                            const void *d_lengths, uint64_t n_reads, uint64_t n_intervals,
                            uint32_t coverage, double not_coverage, yacrd_device_result *out);

/* yacrd_engine_run_device in two halves, so that one host thread can keep batches in flight on
 * several engines of a device (submit on engine A, submit on engine B, wait on A, submit on A ...):
 * the plan / follow-on kernels and the launch gaps of one batch hide behind the
 * sweep of another.  submit enqueues the
 * whole run when the previous run on this engine had the same shape (its class counts size the
 * launches; wait validates them and, in the rare case they do not hold, runs the batch again the
 * synchronous way) and otherwise simply runs it to the end.  The inputs must stay valid until
 * wait returns; between submit and wait the engine accepts no other call. */
int yacrd_engine_submit_device(yacrd_engine *e, const void *d_offsets, const void *d_intervals,
                               const void *d_lengths, uint64_t n_reads, uint64_t n_intervals,
                               uint32_t coverage, double not_coverage);
int yacrd_engine_wait(yacrd_engine *e, yacrd_device_result *out);

/* The submit / wait loop over a LIST of device-resident batches, kept on this side of the ABI (a
 * streaming host that hands over many batches pays one call, not two per batch): batch i runs on
 * engines[i % n_engines], all on one device, up to n_engines batches in flight.  `done`, when given,
 * is called from the calling thread once per batch, in order, after its wait and before its engine
 * is used again — the place to consume the batch's device-resident result (yacrd_engine_fetch) —
 * and a non-zero return stops the loop (YACRD_EINVAL).  The replacement for the batch loop of
 * FromOverlap::compute_all_bad_part (src/stack.rs:143-162) when the overlaps already sit in HBM. */
typedef struct yacrd_device_batch {
    const void *d_offsets, *d_intervals, *d_lengths;
    uint64_t n_reads, n_intervals;
    uint32_t coverage;
    double not_coverage;
} yacrd_device_batch;
typedef int (*yacrd_batch_done_fn)(void *user, uint32_t batch, yacrd_engine *e, const yacrd_device_result *res);
int yacrd_engines_run_device_batches(yacrd_engine *const *engines, uint32_t n_engines,
                                     const yacrd_device_batch *batches, uint32_t n_batches,
                                     yacrd_batch_done_fn done, void *user, yacrd_device_result *last);

/* yacrd_engine_run in two halves for HOST inputs: submit validates the CSR, enqueues H2D + the whole
 * run on the engine's stream and returns; collect waits and brings the result home.  With two
 * engines per GPU a caller keeps PCIe and the kernels busy at the same time (batch k+1 crosses PCIe
 * while batch k is swept) — the batch loop of FromOverlap::compute_all_bad_part
 * (src/stack.rs:143-162) as a pipeline.  Inputs should come from yacrd_pinned_alloc (direct DMA,
 * ~55 GB/s; they must then stay valid until collect returns); pageable inputs are staged through
 * the engine's pinned bounce buffers before submit returns.  Like submit_device, the run is only
 * left in flight when the previous run on this engine had the same shape; otherwise submit runs it
 * to the end and collect just fetches. */
int yacrd_engine_submit(yacrd_engine *e, const uint64_t *offsets, const uint32_t *intervals,
                        const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                        double not_coverage);
int yacrd_engine_collect(yacrd_engine *e, yacrd_result *out);

/* Page-locked host memory (hipHostMalloc) for inputs: the engine recognises it and moves it over
 * PCIe by direct DMA instead of staging.  NULL on failure. */
void *yacrd_pinned_alloc(size_t bytes);
void yacrd_pinned_free(void *p);

/* ---- streaming ingest: overlap records cross PCIe while the parser is still running -------------
 * The north star's "streams it to HBM via pinned hipMemcpyAsync".  The reference hands the engine
 * whole reads (MapReads2Ovl, src/reads2ovl/mod.rs:41) only after the last line is parsed
 * (FullMemory::get_overlaps, src/reads2ovl/fullmemory.rs:46-50); here the parser threads fill
 * pinned buffers with overlap RECORDS (both reads of a PAF/M4 line, src/reads2ovl/mod.rs:108-109)
 * and every full buffer goes to HBM on a copy stream at once, double-buffered.  When the parser is
 * done, yacrd_stream_finish builds the CSR on the GPU (count -> scan -> scatter, the grouping
 * FullMemory::add_overlap_and_length does per line, src/reads2ovl/fullmemory.rs:82-90) and runs the
 * engine on it: parse || H2D, then GPU CSR build + kernels + D2H (all sub-millisecond per 10 M
 * intervals).  Reads are named by 32-bit handles the caller chooses while parsing; `handle_map`
 * translates them to final read ids at finish (NULL = handles are read ids). */
#ifndef YACRD_OVL_REC_DEFINED
#define YACRD_OVL_REC_DEFINED
typedef struct {
    uint32_t a, b;   /* handles of the two reads of an overlap line */
    uint32_t sa, ea; /* interval on read a (PAF cols 3-4, src/io.rs:23-34) */
    uint32_t sb, eb; /* interval on read b (PAF cols 8-9) */
} yacrd_ovl_rec;
/* Where a parser puts its records (implemented by yacrd_stream; consumed by
 * yacrd_ingest_stream in yacrd_host.h).  Both calls may come from several threads at once. */
typedef struct {
    void *ctx;
    /* a buffer of *capacity records to fill; blocks while all buffers are in flight */
    int (*acquire)(void *ctx, yacrd_ovl_rec **buf, uint64_t *capacity);
    /* hand a buffer back with n_records filled (0 allowed): its copy to HBM starts now */
    int (*commit)(void *ctx, yacrd_ovl_rec *buf, uint64_t n_records);
} yacrd_rec_sink;
#endif

typedef struct yacrd_stream yacrd_stream;
/* chunk_records: records per pinned buffer (0 = 131072, 3 MiB); n_buffers: 0 = 2 per usable CPU + 2 */
int yacrd_stream_open(yacrd_engine *e, uint64_t chunk_records, uint32_t n_buffers, yacrd_stream **out);
int yacrd_stream_sink(yacrd_stream *s, yacrd_rec_sink *sink);
int yacrd_stream_acquire(yacrd_stream *s, yacrd_ovl_rec **buf, uint64_t *capacity);
int yacrd_stream_commit(yacrd_stream *s, yacrd_ovl_rec *buf, uint64_t n_records);
/* All records are in.  handle_map[n_handles] (or NULL), lengths[n_reads]: builds the CSR in HBM,
 * runs the engine (blocking) and returns the host result like yacrd_engine_run.  The stream is
 * empty again afterwards — on success AND on every error return — and can take the next file; the two
 * exceptions are calls that are refused before anything is touched (YACRD_EINVAL: a batch pending on the
 * engine, a buffer a parser still holds): fix the cause, then yacrd_stream_reset (the group's finish
 * clears every device when any of its streams failed). */
int yacrd_stream_finish(yacrd_stream *s, const uint32_t *handle_map, uint64_t n_handles,
                        const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                        double not_coverage, yacrd_result *out);
typedef struct {
    uint64_t n_records;  /* overlap records of the last finished stream */
    uint64_t h2d_bytes;  /* bytes the copy stream moved */
    float h2d_busy_ms;   /* sum of the DMA durations (HIP events around each buffer's copy) */
    float build_ms;      /* CSR build on the GPU: count + scan + scatter */
    float run_ms;        /* engine run on the built CSR, wall clock incl. its sync */
    float d2h_ms;
} yacrd_stream_stats;
int yacrd_stream_last_stats(const yacrd_stream *s, yacrd_stream_stats *st);
/* Discard every record committed so far (an ingest that failed half way through its file leaves its
 * records in the stream: call this before the stream takes another file).  No buffer may be held. */
int yacrd_stream_reset(yacrd_stream *s);
void yacrd_stream_close(yacrd_stream *s);

/* ---- streaming ingest over several GPUs --------------------------------------------------------
 * The read-partitioned form of the stream (the reference's equivalent is its batch loop over reads,
 * src/stack.rs:143-162, fed by src/reads2ovl/mod.rs:83-113): a read belongs to device
 * yacrd_stream_device_of(handle, N) = handle mod N, a fact known the moment the parser has interned
 * the id, so the group's sink routes every record while the parse is still running — to the device of
 * its read a and, when that is another one, also to the device of its read b (every record crosses
 * PCIe at most twice, whatever N is) — through one yacrd_stream per device.  At the end each device
 * gets its own handle map (its reads numbered densely in first-appearance order, every other read
 * YACRD_HANDLE_ELSEWHERE: csr_build takes only the half of a record that names a read of its own),
 * builds its CSR, runs; the results are merged back into first-appearance order.  No collective.
 * With one engine the sink is the stream's own (no routing, no extra copy). */
#define YACRD_HANDLE_ELSEWHERE 0xFFFFFFFEu /* in a handle map: this read lives on another device */
typedef struct yacrd_stream_group yacrd_stream_group;
uint32_t yacrd_stream_device_of(uint32_t handle, uint32_t n_devices);
int yacrd_stream_group_open(yacrd_engine *const *engines, uint32_t n_engines, uint64_t chunk_records,
                            uint32_t n_buffers, yacrd_stream_group **out);
int yacrd_stream_group_sink(yacrd_stream_group *g, yacrd_rec_sink *sink);
/* like yacrd_stream_finish; handle_map / lengths are the GLOBAL ones (handle -> first-appearance id) */
int yacrd_stream_group_finish(yacrd_stream_group *g, const uint32_t *handle_map, uint64_t n_handles,
                              const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                              double not_coverage, yacrd_result *out);
/* stats of device `index`'s stream and the number of reads it owned in the last finish */
int yacrd_stream_group_last_stats(const yacrd_stream_group *g, uint32_t index, yacrd_stream_stats *st,
                                  uint64_t *n_reads_owned);
int yacrd_stream_group_reset(yacrd_stream_group *g);
void yacrd_stream_group_close(yacrd_stream_group *g);

/* ---- PAF text -> read types with the parse on the GPU ------------------------------------------------
 * Reads2Ovl::init_paf (src/reads2ovl/mod.rs:83-113) + FullMemory (src/reads2ovl/fullmemory.rs:82-90) +
 * compute_all_bad_part in one call: the host only moves the text (pread chunks -> pinned buffers ->
 * hipMemcpyAsync), the device parses it (nine tab-separated columns as src/io.rs:23-34 names them), interns the
 * ids, numbers the reads by first appearance (a read's length = the first one seen), builds the CSR and runs
 * the engine.  `reads` receives what the report and the editors need to name the reads (host arrays, released
 * with yacrd_reads_free).  Plain PAF files only; returns YACRD_EFALLBACK (nothing else happened) for whatever
 * only the host parser handles — a '"' or a lone CR anywhere (csv quoting / record rules), a 0x integer, a
 * malformed line (the host parser words the error), a read length beyond u32, a file that is not regular:
 * the caller then takes yacrd_ingest_stream + yacrd_stream_finish. */
typedef struct {
    uint64_t n_reads;
    uint64_t n_records;  /* overlap lines */
    uint32_t *lengths;   /* [n_reads] */
    uint64_t *name_off;  /* [n_reads + 1] */
    char *names;         /* name_off[n_reads] bytes, reads in first-appearance order */
} yacrd_reads;
typedef struct {
    uint64_t text_bytes, n_records, n_reads;
    float text_ms;   /* file -> pinned -> HBM (wall clock) */
    float parse_ms;  /* scan + parse + id table on the device */
    float build_ms;  /* numbering, names, CSR */
    float run_ms;    /* the engine */
    float d2h_ms;
} yacrd_ingest_stats;
int yacrd_engine_ingest_paf(yacrd_engine *e, const char *path, int n_threads, uint32_t coverage, double not_coverage,
                            yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */);
/* The same for either overlap format — format: 0 = by file name like util::get_file_type (src/util.rs:39-55), 1 = PAF,
 * 2 = M4 / MHAP (Reads2Ovl::init_m4, src/reads2ovl/mod.rs:115-145; M4Record, src/io.rs:36-50: twelve space-separated
 * columns; an error rate not written as plain decimal digits is the host parser's: YACRD_EFALLBACK). */
int yacrd_engine_ingest_overlaps(yacrd_engine *e, const char *path, int format, int n_threads, uint32_t coverage,
                                 double not_coverage, yacrd_result *out, yacrd_reads *reads,
                                 yacrd_ingest_stats *stats /* may be NULL */);
/* The same over text that already lies in host memory (format: 1 = PAF, 2 = M4) — what a compressed overlap file is
 * once libyacrd_host has inflated it (yacrd_text_from_file: the reference reads .gz / .bz2 / .xz through niffler like
 * any other file, src/util.rs:57-70).  yacrd_engine_ingest_overlaps itself answers YACRD_EFALLBACK for a file that
 * begins with a gzip / bzip2 / xz magic.  `text` needs no padding; it may be pageable. */
int yacrd_engine_ingest_overlaps_mem(yacrd_engine *e, const char *text, uint64_t n_bytes, int format, int n_threads,
                                     uint32_t coverage, double not_coverage, yacrd_result *out, yacrd_reads *reads,
                                     yacrd_ingest_stats *stats /* may be NULL */);
/* The same with SEVERAL engines (one per GPU; engines that share a device take shares of it) — the N-GPU form of
 * Reads2Ovl::init_paf / init_m4 (src/reads2ovl/mod.rs:83-145) + compute_all_bad_part (src/stack.rs:143-162: reads are
 * independent).  Engine d moves and parses a byte range of the text — over its own PCIe link —, cut on 4 MiB boundaries; a
 * line belongs to the range it STARTS in (the range's mirror reaches one chunk beyond it).  The ranges' read lists (name,
 * first position in the file, first length, intervals: a few dozen bytes per read and range) go to engines[0], which numbers
 * the reads of the whole file by first appearance; every engine rewrites its records to those numbers, the reads are dealt
 * out as contiguous ranges of numbers with about the same number of intervals each, every engine builds the CSR of its
 * reads from the records of all ranges (copied device to device where they live elsewhere: the one exchange step the
 * path has) and sweeps it.  Results, names and lengths as from one engine, bit for bit.  YACRD_EFALLBACK as there (any
 * range's text may ask for the host parser).  A text of fewer than two chunks is engines[0]'s alone. */
int yacrd_engines_ingest_overlaps(yacrd_engine *const *engines, uint32_t n_engines, const char *path, int format, int n_threads,
                                  uint32_t coverage, double not_coverage, yacrd_result *out, yacrd_reads *reads,
                                  yacrd_ingest_stats *stats /* may be NULL */);
int yacrd_engines_ingest_overlaps_mem(yacrd_engine *const *engines, uint32_t n_engines, const char *text, uint64_t n_bytes,
                                      int format, int n_threads, uint32_t coverage, double not_coverage, yacrd_result *out,
                                      yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */);
void yacrd_reads_free(yacrd_reads *r);
/* The device parser keeps its buffers between calls (the text's mirror, the id table, the records: about twice the
 * file's size; a call into warm buffers is 2-3 times faster than one that has to allocate them): this gives them back. */
int yacrd_engine_trim(yacrd_engine *e);

/* filter / extract on an OVERLAP file (Filter::run_paf / run_m4, src/editor/filter.rs:140-228; Extract::run_paf / run_m4,
 * src/editor/extract.rs:144-232) with the decision and the compaction on the GPU (csrc/gpu_edit.hip): the host moves the text
 * to HBM as the device parser does and brings the kept bytes back, segment by segment, while later segments are still on
 * their way.  A record is looked at through its first field and field 5 (PAF, tab-separated) or 1 (M4 / MHAP, space-separated);
 * an id the table does not hold is NotBad (src/stack.rs:164-169); filter keeps a record when both reads are NotBad, extract
 * when one is not.  Kept lines come out in file order, each ended by exactly one '\n'; empty lines vanish.  The bytes are
 * those of libyacrd_host's yacrd_edit_file on the same input and table.
 * The table: names[name_off[r] .. name_off[r + 1]) is read r's id (unique ids: what a detection run and yacrd_report_read
 * hand out), read_type[r] its type.
 * YACRD_EFALLBACK, with nothing written: a '"' or a CR anywhere in the text, a line whose field count differs from the first
 * non-empty line's or is too small to hold the second id, a line that reaches more than 4 MiB beyond its 128 MiB segment, a
 * compressed or non-regular input, an output path that exists and is no regular file (or is the input).  The caller then runs
 * yacrd_edit_file, which knows the csv syntax, the codecs and the reference's messages.  The file form writes beside out_path
 * and renames when the last byte is in.
 * Memory: the run holds the text, as many bytes again and an eighth.  A plain text of more than 128 MiB that finds no such
 * room is edited window by window instead (128 MiB of text at a time in a ring of about 0.55 GB, the same
 * bytes; every form: _mem, _gzip_mem, _gzip_file, and — DESIGN.md 7o — the edit from the mirror and the _resident_ forms,
 * which hold no text ring, and the _bgzf_ forms, whose windows end where members end): a line may then reach 4 MiB into the
 * next window (BGZF in: at most the next window's bytes), one that reaches farther is YACRD_EFALLBACK like the line above.
 * YACRD_EFALLBACK for room is left to a device that does not hold the ring.
 * When in_path is the very file (device, inode, size, mtime) the engine's last yacrd_engine_ingest_overlaps parsed and its mirror
 * is still in HBM, the text is not moved again (stats: mirror_reused = 1).
 * op: YACRD_OP_FILTER (1) or YACRD_OP_EXTRACT (2) of yacrd_host.h; format: 0 = by name, 1 = PAF, 2 = M4 / MHAP; n_threads: copy
 * threads as for yacrd_engine_ingest_overlaps (0 = the default).  The buffers stay with the engine: yacrd_engine_trim. */
typedef struct {
    uint64_t n_reads;
    const uint64_t *name_off; /* [n_reads + 1] */
    const char *names;
    const uint8_t *read_type; /* [n_reads] */
} yacrd_type_table;
typedef struct {
    uint64_t text_bytes, kept_bytes;
    uint64_t n_lines; /* non-empty lines */
    uint64_t n_kept;
    float text_ms;   /* the text into HBM, with the kernels and the way out of all segments but the last behind it */
    float table_ms;  /* the names up, the table built */
    float kernel_ms; /* mark + carry + scan + pack, summed over the segments (device events) */
    float out_ms;    /* the writer's busy time: kept bytes D2H and into the file */
    uint32_t mirror_reused;
} yacrd_edit_stats;
int yacrd_engine_edit_overlaps(yacrd_engine *e, int op, const char *in_path, const char *out_path, int format, int n_threads,
                               const yacrd_type_table *types, yacrd_edit_stats *stats /* may be NULL */);
/* The same over text in host memory (format: 1 or 2), the kept bytes in a buffer of the library's: yacrd_edit_text_free. */
int yacrd_engine_edit_overlaps_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, int format,
                                   const yacrd_type_table *types, char **out, uint64_t *out_bytes,
                                   yacrd_edit_stats *stats /* may be NULL */);
void yacrd_edit_text_free(char *p);

/* ---- gzip output compressed on the GPU (csrc/gpu_deflate.hip, csrc/deflate_block.h) -----------------------------------
 * Text -> a BGZF stream (SAM spec 4.1; every gzip reader reads it as gzip, and it inflates member-parallel): the text is
 * cut into blocks of 65 280 bytes, one workgroup turns a block into one member (LZ77 matches + a dynamic Huffman code
 * built for the block, or a stored block when that does not shrink it; CRC-32 on the device), the members are packed
 * end to end in HBM and the 28-byte EOF member closes the stream.  The bytes are a pure function of the text. */
typedef struct {
    uint64_t in_bytes, out_bytes, n_members;   /* members without the EOF marker */
    uint64_t n_stored;                         /* members written as stored blocks */
    float h2d_ms, kernel_ms, d2h_ms, write_ms; /* kernel_ms from device events, summed over segments */
} yacrd_gzip_stats;

/* host memory in, one BGZF stream out in a buffer of the library's (yacrd_edit_text_free) */
int yacrd_engine_gzip_mem(yacrd_engine *e, const char *data, uint64_t n_bytes,
                          char **out, uint64_t *out_bytes, yacrd_gzip_stats *stats /* may be NULL */);

/* ---- BGZF inflated on the GPU (csrc/gpu_inflate.hip, csrc/inflate_block.h, csrc/bgzf_walk.h) --------------------------
 * The other half: a BGZF stream in host memory -> its text.  The host walks the members (no zlib: `1f 8b 08 04`, the `BC`
 * subfield anywhere in the extra field, BSIZE, the trailer's ISIZE <= 65 536; EOF members anywhere), the stream crosses the
 * link compressed, and one wavefront per member decodes it in LDS — a full RFC 1951 decoder: stored, fixed and dynamic
 * blocks, any number per member — checks the member's CRC-32 and ISIZE against what it produced and stores the text at the
 * member's place.  An empty input and a stream of EOF members give an empty text (a buffer all the same).
 * YACRD_EFALLBACK, with nothing returned: a stream that is not BGZF from its first member to its last (plain gzip; FNAME,
 * FCOMMENT or FHCRC set; a BSIZE beyond the input; bytes after the last member), or any member the decoder does not take —
 * the payload ends early or has bytes left over, block type 3, LEN / NLEN mismatch, over-subscribed or incomplete code
 * lengths (a single distance code of length 1, which zlib writes, passes), a repeat with nothing in front, HLIT / HDIST
 * beyond 286 / 30, length symbols 286-287 or distance symbols 30-31, a distance beyond the bytes produced, output beyond
 * ISIZE or short of it, CRC mismatch.  Stricter than zlib in places, never more lenient: the caller then takes
 * libyacrd_host's reader, which owns the messages.  The engine stays usable.  `out`: yacrd_edit_text_free.  The buffers
 * stay with the engine: yacrd_engine_trim.  Additive: found by the symbol. */
typedef struct {
    uint64_t in_bytes, out_bytes, n_members; /* members as walked, EOF members among them */
    float walk_ms, h2d_ms, kernel_ms /* device events */, d2h_ms;
} yacrd_gunzip_stats;
int yacrd_engine_gunzip_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes,
                            char **out, uint64_t *out_bytes, yacrd_gunzip_stats *st /* may be NULL */);

/* ---- plain gzip inflated on the GPU (csrc/gpu_gunzip_stream.hip, csrc/inflate_stream.h, csrc/gzip_walk.h) ------------
 * ONE plain gzip member — what `gzip` and `minimap2 | gzip` write — in host memory -> its text.  yacrd_engine_gunzip_mem
 * and every _bgzf_ form keep refusing it; this is a route of its own.  The host walks the header (`1f 8b 08 FLG`, reserved
 * FLG bits zero; FEXTRA, FNAME, FCOMMENT and FHCRC skipped), the member crosses the link compressed, and the deflate stream
 * is decoded in parallel in five steps, each its own launches: block starts are FOUND per chunk of compressed
 * bytes (dynamic, non-final headers, judged in registers), the spans between them are SIZED without storing a byte and
 * chained from bit 0 by the host (a guess the chain does not confirm is dropped; a block start the chain proves and no span
 * begins on is sized in one more round), decoded again into 16-bit SYMBOLS where a byte from in front of its span is a
 * marker, the last 32 768 symbols of every span are resolved in order (WINDOWS), and the BYTES go out position-parallel with
 * the CRC-32 summed on the way.  ISIZE is checked before a byte is stored, the CRC-32 behind the last one.  A wrong guess
 * costs time, never bytes.  YACRD_EFALLBACK, with nothing returned and the engine usable: not one gzip member (a header
 * cut short, reserved bits, fewer than header + 8 bytes); concatenated members, trailing bytes or a BGZF stream ("bytes left
 * over": the final block must end in the payload's last byte); yacrd_engine_gunzip_mem's list of payload faults; more than
 * 64 wrong block starts; a span (the stretch one wavefront decodes: an all-stored or all-fixed stream is one) of more than 32 MiB compressed or 64 MiB of text; a payload beyond 2^40 bytes;
 * text + 2 x text + compressed bytes beyond the device's free memory.  Never more lenient than zlib.  The caller then takes
 * libyacrd_host's reader, which owns the messages.  `out`: yacrd_edit_text_free.  The buffers stay with the engine:
 * yacrd_engine_trim.  Additive: found by the symbol. */
typedef struct {
    uint64_t in_bytes, out_bytes, n_chunks;
    uint64_t n_spans;        /* true spans: the pieces decoded in parallel */
    uint64_t n_false_starts; /* finds the chain stepped over */
    uint64_t rounds;         /* launches of the sizing step: 1, and one per proven start that had no span */
    uint64_t n_blocks;
    float find_ms, size_ms, symbols_ms, windows_ms, bytes_ms; /* device events */
    float h2d_ms, d2h_ms;
} yacrd_gunzip_stream_stats;
int yacrd_engine_gunzip_stream_mem(yacrd_engine *e, const char *gz, uint64_t n_bytes,
                                   char **out, uint64_t *out_bytes, yacrd_gunzip_stream_stats *st /* may be NULL */);

/* yacrd_engine_ingest_overlaps_mem and yacrd_engine_ingest_report_mem over a BGZF stream as it lies in host memory (read
 * or mapped: no host inflate).  The host walks the members, the COMPRESSED bytes go up in the mover's 4 MiB chunks, and for
 * every 128 MiB of them that has landed the members that have become complete are decoded by one launch on the engine's
 * stream (csrc/bgzf_plan.h names them); the parser's / the reader's scan runs over every 128 MiB of TEXT that is whole behind
 * those launches, as it does over plain text that lands.  `out`, `reads` and the resident table are bit for bit those of the
 * _mem form on the inflated text.  stats->text_bytes is the inflated size, text_ms covers the way up and the inflate; `us`
 * as in the editors' _bgzf_ forms: walk_ms, h2d_ms (the compressed bytes), kernel_ms (the decoder's launches, by device
 * events), d2h_ms 0.  YACRD_EFALLBACK, with nothing returned and the engine usable: a stream that is not BGZF, a member the
 * decoder does not take (yacrd_engine_gunzip_mem's list; the decoder's status is read before anything is sized from the text,
 * and wins over what the parser made of it), the _mem forms' own causes in the text, a text beyond the device's free memory
 * (which now also holds the compressed bytes and the member table).  The caller then inflates on the host
 * (yacrd_text_from_file) and takes the _mem form or the host parser.  Additive: found by the symbol. */
int yacrd_engine_ingest_overlaps_bgzf_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes, int format /* 1 PAF, 2 M4 */,
                                          int n_threads, uint32_t coverage, double not_coverage, yacrd_result *out,
                                          yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */,
                                          yacrd_gunzip_stats *us /* may be NULL */);
int yacrd_engine_ingest_report_bgzf_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes, int n_threads, double not_coverage,
                                        yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */,
                                        yacrd_gunzip_stats *us /* may be NULL */);

/* filter / extract with gzip out: the kept bytes of yacrd_engine_edit_overlaps_mem deflated where the pack pass leaves them
 * in HBM, so that only members cross the link and reach the file.  `text` is the overlap text in host memory, already
 * inflated (format 1 = PAF / 2 = M4, MHAP): this library links no zlib and inflates BGZF only for the sequence editors
 * (yacrd_engine_gunzip_mem below the editors' _bgzf_ forms); here the caller inflates (libyacrd_host's
 * yacrd_text_from_file is member-parallel for BGZF).  The decision and the kept bytes are those of
 * yacrd_engine_edit_overlaps_mem; the result is ONE BGZF stream, byte for byte what yacrd_engine_gzip_mem returns for the
 * kept bytes: blocks of 65 280 bytes counted from the start of the kept stream, the EOF member last (nothing kept: the EOF
 * member alone).  It does not depend on the editor's segments, on threads or on timing.  As soon as a segment is packed,
 * its whole blocks are encoded on a stream of their own while later segments are moved, marked and packed; the tail of
 * fewer than 65 280 bytes waits for the next segment.  Every buffer is taken before the first segment is handed over
 * (YACRD_ENOMEM: nothing was written, nothing is left behind); they stay with the engine (yacrd_engine_trim).
 * YACRD_EFALLBACK for the causes of the plain form; found in a later segment, members of earlier ones may already have
 * left the device: the buffer is freed, the file beside out_path removed, nothing is left at out_path.
 * es as for the plain form (out_ms: the writer thread's busy time, members D2H and into the file); gs: in_bytes ==
 * es->kept_bytes, kernel_ms from device events around the encode and pack launches, summed over the batches; d2h_ms
 * holds the writer's waits for the encoder as well.  The file form writes beside out_path and renames when the EOF member
 * is in; the memory form returns a buffer of the library's (yacrd_edit_text_free). */
int yacrd_engine_edit_overlaps_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, int format,
                                        const yacrd_type_table *types, char **out, uint64_t *out_bytes,
                                        yacrd_edit_stats *es /* may be NULL */, yacrd_gzip_stats *gs /* may be NULL */);
int yacrd_engine_edit_overlaps_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, int format,
                                         const yacrd_type_table *types, const char *out_path,
                                         yacrd_edit_stats *es /* may be NULL */, yacrd_gzip_stats *gs /* may be NULL */);
/* filter / extract on a BGZF overlap file as it is: `bgzf`, n_bytes is the COMPRESSED file in host memory (read or mapped);
 * the host inflates nothing.  The compressed bytes go up once, the members of every landed segment are inflated into the
 * editor's text buffer (yacrd_engine_ingest_overlaps_bgzf_mem's mover), and every whole segment of TEXT is marked, scanned
 * and packed behind the launches that decoded it.  format 1 = PAF / 2 = M4, MHAP.  gzip_out 0: the kept bytes, those of
 * yacrd_engine_edit_overlaps_mem on the inflated text; gzip_out 1: ONE BGZF stream, byte for byte what
 * yacrd_engine_edit_overlaps_gzip_mem returns for that text.  The host decodes, for the two things the plan must know before
 * the first launch (the first non-empty line's field count; whether the text ends in a newline), the stream's first members
 * — at most 1 MiB of text, no further than that line's end — and its last one.
 * es->text_bytes is the inflated size; us: walk_ms, h2d_ms of the compressed bytes, kernel_ms of the decoder by device events,
 * d2h_ms 0; gs is zero with gzip_out 0.
 * YACRD_EFALLBACK — nothing written, nothing left at or beside out_path, es / gs / us zeroed, the engine usable — for a
 * stream that is not BGZF, a member the decoder does not take (its status word is read before anything the editor's kernels
 * made of the text, and wins: kept bytes of earlier segments may have reached the sink by then, so the memory form frees its
 * buffer and the file form removes the file beside out_path), a first line longer than the host's sample, the plain forms'
 * own causes in the text, and a text beyond the device's free memory.  The file form's rules for out_path are those of
 * yacrd_engine_edit_overlaps_gzip_file.  Additive: found by the symbol. */
int yacrd_engine_edit_overlaps_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, int format,
                                        const yacrd_type_table *types, int gzip_out /* 0 | 1 */, char **out, uint64_t *out_bytes,
                                        yacrd_edit_stats *es /* may be NULL */, yacrd_gzip_stats *gs /* may be NULL */,
                                        yacrd_gunzip_stats *us /* may be NULL */);
int yacrd_engine_edit_overlaps_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, int format,
                                         const yacrd_type_table *types, int gzip_out /* 0 | 1 */, const char *out_path,
                                         yacrd_edit_stats *es /* may be NULL */, yacrd_gzip_stats *gs /* may be NULL */,
                                         yacrd_gunzip_stats *us /* may be NULL */);
/* filter / extract on the overlap text that the engine's last successful overlap ingest left in HBM: nothing goes up
 * (es->mirror_reused 1, text_ms 0); the bytes are those of the forms above.  The text is recorded, with its size, its format
 * and the two things the plan asks of it, by every one-engine overlap ingest that leaves the whole text in HBM:
 * yacrd_engine_ingest_overlaps, _overlaps_mem and _overlaps_bgzf_mem (a group of several engines leaves none).  Whatever
 * rewrites or frees that text — the next ingest of any kind, whether it succeeds or not, yacrd_engine_trim — ends it; the
 * report writer and the editors leave it alone.  A text that came from memory or from a BGZF stream carries no file identity:
 * yacrd_engine_edit_overlaps never takes it for its file.  With no such text: YACRD_EINVAL, "no overlap text is resident" —
 * no fallback, the caller's logic is wrong.  YACRD_EFALLBACK, nothing written: the plain forms' own causes in the text, no
 * device memory, and a resident text whose ingest could not take the plan's two facts (a BGZF text whose first line is longer
 * than the 1 MiB the host samples; a read error in the file): the host loop's.  Additive: found by the symbol. */
int yacrd_engine_edit_overlaps_resident_mem(yacrd_engine *e, int op, const yacrd_type_table *types, int gzip_out /* 0 | 1 */,
                                            char **out, uint64_t *out_bytes, yacrd_edit_stats *es /* may be NULL */,
                                            yacrd_gzip_stats *gs /* may be NULL */);
int yacrd_engine_edit_overlaps_resident_file(yacrd_engine *e, int op, const yacrd_type_table *types, int gzip_out /* 0 | 1 */,
                                             const char *out_path, yacrd_edit_stats *es /* may be NULL */,
                                             yacrd_gzip_stats *gs /* may be NULL */);

#ifndef YACRD_BYTE_SINK_DEFINED
#define YACRD_BYTE_SINK_DEFINED
typedef struct {
    void *ctx;
    int (*write)(void *ctx, const char *p, uint64_t n); /* non-zero = stop */
} yacrd_byte_sink;
#endif
/* A file written as it is produced: bytes arrive through write(), leave as BGZF.  write() copies into a pinned segment
 * buffer; a full segment (segment_bytes, rounded to whole blocks; 0 = 512 blocks) goes to the device and is compressed
 * while the caller fills the other of two buffers; its members are fetched and appended to the file when the next segment
 * is due.  n_buffers is accepted for callers that size a deeper pipeline and is not used yet: one segment is in flight at
 * a time, two buffers are pinned whatever it says.  The result does not depend on segment_bytes or on how the caller slices its writes.  All
 * device and pinned memory is taken in open (YACRD_ENOMEM: nothing was written, the caller can fall back); the buffers
 * stay with the engine (yacrd_engine_trim returns them once the writer is gone).  The file is written beside out_path
 * and renamed in close.  One writer per engine at a time; the engine runs nothing else meanwhile. */
typedef struct yacrd_gzip_writer yacrd_gzip_writer;
int yacrd_gzip_writer_open(yacrd_engine *e, const char *out_path, uint64_t segment_bytes /* 0 = default */,
                           uint32_t n_buffers /* 0 = default */, yacrd_gzip_writer **out);
int yacrd_gzip_writer_write(yacrd_gzip_writer *w, const char *p, uint64_t n);
/* a sink whose write() is yacrd_gzip_writer_write (for libyacrd_host's yacrd_edit_file_to); valid while the writer lives */
int yacrd_gzip_writer_sink(yacrd_gzip_writer *w, yacrd_byte_sink *sink);
/* flush, EOF marker, rename; the writer is gone afterwards whatever is returned (on failure nothing is left at out_path) */
int yacrd_gzip_writer_close(yacrd_gzip_writer *w, yacrd_gzip_stats *stats /* may be NULL */);
void yacrd_gzip_writer_abort(yacrd_gzip_writer *w); /* nothing is left at out_path */

/* ---- a `.yacrd` report read on the GPU (csrc/gpu_report.hip) -------------------------------------------------------------
 * FromReport (src/stack.rs:176-257) behind src/main.rs:43-60: a report stands in for the overlap file, detection is skipped,
 * the regions come from the report and type_of_read is redone with this run's not_coverage.  The host only moves the text to
 * HBM; the device cuts the lines, parses `type \t id \t len \t len_i,begin_i,end_i;...`, interns the ids (an id seen again
 * REPLACES the earlier row's length and regions and keeps its position), numbers the reads by first appearance, fills the
 * region CSR and classifies it where it lies.  `out` holds bad_offsets, bad_regions and read_type — exactly what libyacrd_host's
 * yacrd_report_read + yacrd_report_get and yacrd_engine_classify give —, `reads` the names, name_off and lengths
 * (n_records: the non-empty lines); released with yacrd_result_free / yacrd_reads_free.  stats: text_ms the text into HBM with
 * the line count behind it, parse_ms parse + id table + numbering, build_ms gather + scans + fill + types, run_ms 0.
 * YACRD_EFALLBACK, with nothing returned: a compressed or non-regular file (inflate it and take the _mem form), any line the
 * host reader calls corrupt (fewer than four columns, a length or a position that is not plain decimal digits or is beyond
 * 2^32 - 1, a piece with fewer than two commas, a body that ends in ';'), a report beyond the device's free memory.  The
 * caller then runs yacrd_report_read, which words the error with its line number.  The _mem form takes pageable memory and
 * needs no padding.  The buffers stay with the engine: yacrd_engine_trim. */
int yacrd_engine_ingest_report(yacrd_engine *e, const char *path, int n_threads, double not_coverage,
                               yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */);
int yacrd_engine_ingest_report_mem(yacrd_engine *e, const char *text, uint64_t n_bytes, int n_threads, double not_coverage,
                                   yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats /* may be NULL */);

/* ---- a `.yacrd` report written on the GPU (csrc/gpu_report_write.hip) ----------------------------------------------------
 * The report of src/editor/mod.rs:61-83, byte for byte what libyacrd_host's yacrd_report_write writes for the same arrays: one
 * line per read in table order, `{NotBad|Chimeric|NotCovered} \t id \t len \t piece;piece;... \n`, a piece
 * `{end - begin as u32, wrapping},{begin},{end}`, an id any bytes.  The device sizes every head and every piece, scans the
 * sizes and formats the whole text in one buffer in HBM (a thread per read, a thread per region); the text then comes home
 * in segments through two pinned buffers, segment i + 1 crossing the link while segment i is written.  The file form
 * writes beside out_path and renames when the last byte is in; the memory form returns a buffer of the library's
 * (yacrd_edit_text_free).  The bytes do not depend on the segment size.
 * t == NULL, the RESIDENT form: the arrays are read where the engine's last ingest left them in HBM, nothing is uploaded —
 * after yacrd_engine_ingest_paf / _overlaps[_mem], the N-engine forms called with ONE engine, or
 * yacrd_engine_ingest_report[_mem]; any run, submit, stream finish, ingest, classify or yacrd_engine_trim called on the engine
 * since — whether it succeeded or not, in every form: device, batches, partitioned, group — and there is no such table:
 * YACRD_EFALLBACK.  Otherwise the table's seven arrays are uploaded first.
 * YACRD_EFALLBACK, with nothing written and nothing left behind: a read_type beyond 2 (found on the device), bad_offsets or
 * name_off that do not rise from 0 to their totals, an id of 2^31 bytes, 2^31 reads or regions, an out_path that exists and is no
 * regular file or beside which no file can be created (it is created before anything is formatted), an existing out_path
 * with further hard links or one that may not be written (the rename would replace what yacrd_report_write truncates in
 * place; an existing file's mode is kept).  The caller then runs yacrd_report_write, which owns the messages.
 * YACRD_ENOMEM: the text's buffer did not fit; nothing was written.  The buffers stay with the engine: yacrd_engine_trim. */
typedef struct { /* host arrays, as yacrd_reads + yacrd_result hold them */
    uint64_t n_reads;
    const uint64_t *name_off; /* R+1 */
    const char *names;
    const uint32_t *lengths;      /* R */
    const uint64_t *bad_offsets;  /* R+1 */
    const uint32_t *bad_regions;  /* 2*G */
    const uint8_t *read_type;     /* R */
} yacrd_report_table;
typedef struct {
    uint64_t n_reads, n_regions, text_bytes;
    float up_ms;     /* the table's upload (device events; ~0 for the resident form) */
    float kernel_ms; /* size + scan + emit (device events) */
    float out_ms;    /* the writer's busy time: segments into the file or the buffer */
    uint32_t resident;
} yacrd_report_write_stats;
int yacrd_engine_write_report(yacrd_engine *e, const yacrd_report_table *t /* NULL = resident */, const char *out_path,
                              yacrd_report_write_stats *st /* may be NULL */);
int yacrd_engine_write_report_mem(yacrd_engine *e, const yacrd_report_table *t /* NULL = resident */, char **out, uint64_t *out_bytes,
                                  yacrd_report_write_stats *st /* may be NULL */);

/* ---- scrubb / split / filter / extract on a FASTQ file on the GPU (csrc/gpu_seq_edit.hip) ------------------------------------
 * The sequence editors of src/editor/{scrubbing,split,filter,extract}.rs on a FASTQ: the text goes to HBM, the device cuts it
 * into lines (record r is lines 4r .. 4r + 3), looks every record's key — the first whitespace token of its name — up in the
 * table, applies the op's rule, sizes the output, scans the sizes and gathers the output in one buffer in HBM: a copied record
 * is the input record's bytes, a cut record `@{name}_{p0}_{p1}[ {desc}]`, that slice of the sequence, `+`, the same slice of
 * the quality.  The bytes are those of libyacrd_host's yacrd_edit_file on the same input and table.
 * op: all four YACRD_OP_* of yacrd_host.h.  t: the table, uploaded by the call (names, lengths, region CSR, types; unique
 * ids); the resident form (t == NULL) is not built: YACRD_EINVAL.
 * YACRD_EFALLBACK, with nothing written and nothing left beside out_path: a text that is not, as a whole, what the host's
 * fast path takes — the line count a multiple of four and the last line ended, no CR anywhere, every header `@name[ desc]`
 * with a name and no blank directly in front of its newline, every third line exactly `+`, sequence and quality of equal
 * length (0 is allowed); a cut position beyond the record's sequence or a region with begin > end (the host words both);
 * 2^31 records or output records; a compressed or non-regular input, or one whose name does not say FASTQ, to the file form;
 * an out_path that is the input or exists and is no regular file.  Memory is no cause for these four forms: a text that does
 * not fit the device's free memory with its output is edited window by window (128 MiB of text at a time, in a ring of
 * buffers: DESIGN 7k), with the same bytes; what is left of it is a single record of more than 128 MiB ("a record longer
 * than a window"), and the ring itself not fitting.  In windows a cause may be found after earlier windows' output has
 * left the device: the file beside out_path is then dropped, the _mem buffer freed, the stats zeroed — nothing written,
 * nothing left beside out_path, as before.  (The BGZF-in forms below hold text and output in HBM whole, and say
 * YACRD_EFALLBACK when they do not fit; FASTA runs in windows like FASTQ: DESIGN 7l.)  The caller then runs yacrd_edit_file, which owns the syntax, the
 * codecs and the messages.  An empty text is an empty output.
 * In windows the stats' counts and bytes are sums over the windows, kernel_ms the sum of the windows' event pairs, text_ms the
 * time this thread spent landing windows, out_ms the writer thread's busy time.
 * The file form writes beside out_path and renames when the last byte is in; buffers of the _mem forms: yacrd_edit_text_free.
 * The gzip forms mirror yacrd_engine_edit_overlaps_gzip_*: `text` is the inflated FASTQ, the finished output is deflated
 * where it lies and only members come home; the result is ONE BGZF stream, byte for byte yacrd_engine_gzip_mem of the plain
 * form's output (nothing kept: the EOF member alone).  The buffers stay with the engine: yacrd_engine_trim. */
typedef struct {
    uint64_t text_bytes, out_bytes;
    uint64_t n_records;     /* of the input */
    uint64_t n_out_records; /* copied records and cut pieces */
    float text_ms;   /* the text into HBM, the segments' line counts behind it */
    float table_ms;  /* the table up, the id table built */
    float kernel_ms; /* lines + scan + index + plan + scans + pieces + copy (device events) */
    float out_ms;    /* the output (or its members) D2H and into the file or the buffer */
} yacrd_seq_edit_stats;
int yacrd_engine_edit_fastq(yacrd_engine *e, int op, const char *in_path, const char *out_path, int n_threads,
                            const yacrd_report_table *t, yacrd_seq_edit_stats *st /* may be NULL */);
int yacrd_engine_edit_fastq_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */);
int yacrd_engine_edit_fastq_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                     char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                     yacrd_gzip_stats *gs /* may be NULL */);
int yacrd_engine_edit_fastq_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                      const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                      yacrd_gzip_stats *gs /* may be NULL */);
/* The BGZF forms mirror the gzip forms argument for argument, with two differences: `bgzf`, n_bytes is the COMPRESSED file in
 * host memory (read or mapped: no host inflate), and a trailing yacrd_gunzip_stats is added.  The compressed bytes go up through
 * the editor's mover into a buffer of their own, yacrd_engine_gunzip_mem's device step inflates the members into the
 * editor's text buffer, and from there the run is the gzip form's: the output is byte for byte that of the gzip form given the
 * inflated text.  Every YACRD_EFALLBACK cause of the gzip form applies unchanged (the text's last byte is looked at on the
 * device, behind the inflate), plus yacrd_engine_gunzip_mem's: not BGZF, or a member not taken.  Nothing is written and
 * nothing is left beside out_path.  us: h2d_ms is the compressed file's way up, kernel_ms the inflate kernel (device
 * events), d2h_ms 0; st->text_ms covers both.  Additive: found by the symbol. */
int yacrd_engine_edit_fastq_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, const yacrd_report_table *t,
                                     char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                     yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stats *us /* may be NULL */);
int yacrd_engine_edit_fastq_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, const yacrd_report_table *t,
                                      const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                      yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stats *us /* may be NULL */);

/* ---- the same on a FASTA file (csrc/gpu_seq_edit.hip) ---------------------------------------------------------------------
 * A line that begins with '>' starts a record; its name is the header up to the first blank, tab or form feed, its
 * description everything behind that one byte, its sequence every line up to the next '>' line, concatenated (blank lines
 * add nothing; blank lines in front of the first header are skipped).  The key is the whole name.  Every record that goes out
 * is written again: a copied record is `>{name}[ {desc}]` (the separator a blank, dropped with an empty description), a cut
 * piece `>{name}_{p0}_{p1}` without description; the sequence or its slice follows 80 bases a line, nothing for an empty one.
 * The bytes are those of yacrd_edit_file on the same input and table.  The device marks the header lines, scans them into
 * record ordinals and the other lines' lengths into base ordinals, plans per record and gathers per 4 KiB of output: an output
 * base is found in the input by arithmetic when its record's lines have one width, else by a search over the record's lines.
 * Arguments, stats, the file form's rename, the _mem buffers and the gzip forms' stream: as the four calls above.
 * YACRD_EFALLBACK, with nothing written and nothing left beside out_path: a CR anywhere; a last line without its newline; a
 * line that is not blank in front of the first header; a header without a name (`>`, `> desc`: stricter than the host, which
 * writes them back); a cut position beyond the record's sequence or a region with begin > end; 2^31 records or output records;
 * a record, or a read's output, of 0xFF000000 bytes or more; to the file form a compressed or non-regular input, a name that
 * yacrd_edit_file would not take for FASTA (.fastq / .fq / .paf / .m4 / .mhap / .yacrd win over .fa) and an out_path that is
 * the input or no regular file.  Memory: a text that does not fit the device's free memory with its line tables (32 bytes a
 * line) and its output is edited window by window, as for FASTQ above: a window completes the records in front
 * of its last '>' line and hands the rest to the next; what is left is a record of more than 128 MiB ("a record longer than
 * a window"), a ring or a window's tables that do not fit, and the BGZF-in forms, which hold text and output whole.
 * An empty text and a text of blank lines are an empty output. */
int yacrd_engine_edit_fasta(yacrd_engine *e, int op, const char *in_path, const char *out_path, int n_threads,
                            const yacrd_report_table *t, yacrd_seq_edit_stats *st /* may be NULL */);
int yacrd_engine_edit_fasta_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */);
int yacrd_engine_edit_fasta_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                     char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                     yacrd_gzip_stats *gs /* may be NULL */);
int yacrd_engine_edit_fasta_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n_bytes, const yacrd_report_table *t,
                                      const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                      yacrd_gzip_stats *gs /* may be NULL */);
/* ... and the BGZF forms, as for FASTQ */
int yacrd_engine_edit_fasta_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, const yacrd_report_table *t,
                                     char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                     yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stats *us /* may be NULL */);
int yacrd_engine_edit_fasta_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, const yacrd_report_table *t,
                                      const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                      yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stats *us /* may be NULL */);
/* The plain-gzip forms, for FASTQ and FASTA: the _bgzf_ forms' arguments, with `gz`, n_bytes ONE plain gzip member in host
 * memory and yacrd_gunzip_stream_stats in place of yacrd_gunzip_stats.  The member goes up and is sized and chained on the
 * device (yacrd_engine_gunzip_stream_mem's first steps) before anything is made beside out_path; its symbols, windows and
 * bytes go into the editor's text buffer, the decoder's status and the CRC-32 are read before anything is sized from the
 * text, and from there the run is the gzip form's: the output is byte for byte that of the gzip form given the inflated
 * text.  The whole-text run only: a text that would run in windows (it finds no room whole, or yacrd_debug_seq_window names
 * a window it outgrows) is YACRD_EFALLBACK, as are the gzip form's causes and yacrd_engine_gunzip_stream_mem's.  Nothing is
 * written and nothing is left beside out_path, and a call that fails frees the compressed bytes and the symbol scratch it
 * took at once: the host route that follows finds the device memory it would have found without the attempt.  ss->d2h_ms
 * is 0.  Additive: found by the symbol. */
int yacrd_engine_edit_fastq_gz_mem(yacrd_engine *e, int op, const char *gz, uint64_t n_bytes, const yacrd_report_table *t,
                                   char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                   yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stream_stats *ss /* may be NULL */);
int yacrd_engine_edit_fastq_gz_file(yacrd_engine *e, int op, const char *gz, uint64_t n_bytes, const yacrd_report_table *t,
                                    const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                    yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stream_stats *ss /* may be NULL */);
int yacrd_engine_edit_fasta_gz_mem(yacrd_engine *e, int op, const char *gz, uint64_t n_bytes, const yacrd_report_table *t,
                                   char **out, uint64_t *out_bytes, yacrd_seq_edit_stats *st /* may be NULL */,
                                   yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stream_stats *ss /* may be NULL */);
int yacrd_engine_edit_fasta_gz_file(yacrd_engine *e, int op, const char *gz, uint64_t n_bytes, const yacrd_report_table *t,
                                    const char *out_path, yacrd_seq_edit_stats *st /* may be NULL */,
                                    yacrd_gzip_stats *gs /* may be NULL */, yacrd_gunzip_stream_stats *ss /* may be NULL */);

/* Copy the last device result to host (allocates like yacrd_engine_run). */
int yacrd_engine_fetch(yacrd_engine *e, yacrd_result *out);

int yacrd_engine_last_timing(const yacrd_engine *e, yacrd_timing *t);
/* Sums of the float fields over the runs since the last reset (count fields are those of the
 * last run), and how many runs: lets a caller time K runs without K round trips. */
int yacrd_engine_timing_total(yacrd_engine *e, yacrd_timing *sum, uint64_t *n_runs, int reset);

/* Elapsed time of an EMPTY event bracket on the engine's stream (mean of 32): what the two
 * hipEventRecord calls add to a class_ms / fused_ms value.  Lets a caller report the kernel's own
 * duration (bracket - overhead) next to the raw bracket; rocprofv3 --kernel-trace gives the same
 * figure from the dispatch timestamps. */
int yacrd_engine_event_overhead(yacrd_engine *e, float *ms);

/* Read-id partitioning for multi-GPU: cuts[n_parts+1], contiguous read
 * ranges balanced by interval count; reads are independent so there is no exchange step. */
int yacrd_partition_reads(const uint64_t *offsets, uint64_t n_reads, uint32_t n_parts,
                          uint64_t *cuts);

/* Read-partitioned run over several GPUs of one node: contiguous read ranges from
 * yacrd_partition_reads(), one host thread per engine (one engine per device; the same device
 * may appear twice, useful for testing), no collective — results are concatenated in read order,
 * so the output is identical to a single-engine run. */
int yacrd_engines_run_partitioned(yacrd_engine *const *engines, uint32_t n_engines,
                                  const uint64_t *offsets, const uint32_t *intervals,
                                  const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                                  double not_coverage, yacrd_result *out);

/* Standalone classification of an existing region CSR (the reference calls type_of_read
 * again in every editor, e.g. src/editor/scrubbing.rs:181).  Host buffers in, host out. */
int yacrd_engine_classify(yacrd_engine *e, const uint64_t *bad_offsets,
                          const uint32_t *bad_regions, const uint32_t *lengths,
                          uint64_t n_reads, double not_coverage, uint8_t *read_type);

#ifdef __cplusplus
}
#endif
#endif
