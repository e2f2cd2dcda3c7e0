/*
 * yacrd_engine_debug.h — A/B and test switches for yacrd_engine_cfg.flags.  Not part of the drop-in
 * boundary (include/yacrd_engine.h): they pin one kernel family or one build of a launch so that the
 * tests can run every path against the oracle and tools/ can measure one against the other.  The product
 * path is flags = 0 (plus the timing flags of yacrd_engine.h).
 */
#ifndef YACRD_ENGINE_DEBUG_H
#define YACRD_ENGINE_DEBUG_H

#include "yacrd_engine.h"

/* route every read through the fully general (arbitrary-input) kernel; testing only */
#define YACRD_F_FORCE_GENERAL 1u
/* use the LDS-sort kernel for the small class instead of the register-sort kernel; A/B only */
#define YACRD_F_FORCE_LDS_SORT 2u
/* (4u was YACRD_F_XLANE_DS, 128u YACRD_F_NO_FUSED_LAUNCH, 16384u YACRD_F_SWEEP_TURNS: A/B switches whose paths are gone;
 * the bits are not reused and, like every unknown bit, ignored) */
/* no four-reads-per-wavefront row layout: every small read gets a whole wavefront; A/B only */
#define YACRD_F_WAVE_ONLY 8u
/* no two-reads-per-wavefront layout for reads of 129..256 intervals; A/B only */
#define YACRD_F_NO_HALVES 16u
/* always wait for the plan's class counts (no prediction from the previous run); A/B only */
#define YACRD_F_NO_PREDICTION 64u
/* sort every event: skip the coverage pre-filter (register-sort and LDS classes; A/B, tests) */
#define YACRD_F_NO_PREFILTER 256u
/* count the reads the pre-filter thinned (yacrd_timing.prefiltered_reads); one global atomic per
 * read, so only for tests */
#define YACRD_F_COUNT_PREFILTERED 512u
/* the fused launch of the register-sort classes never runs the healthy-read screen (by default it does
 * from 4 M intervals in the classes R16 + H16 on, unless the previous batches failed the screen too
 * often); 8192: it always does; A/B, tests */
#define YACRD_F_NO_DEFER 4096u
#define YACRD_F_ALWAYS_DEFER 8192u
/* the screen takes one / two groups of list entries per wavefront whatever the
 * launch's size (default: two from 40 M intervals on, i.e. inputs outside the Infinity Cache); tests, A/B */
#define YACRD_F_SCREEN_ITEMS_1 262144u
#define YACRD_F_SCREEN_ITEMS_2 524288u
/* the workgroup classes (513 .. 16 384 intervals) run the screen and its fallback as separate launches (round 3's
 * chain) instead of the persistent screen_wg_fused_kernel; A/B, tests */
#define YACRD_F_NO_FUSED_SCREEN 1048576u
/* the workgroup classes go through a screen of one read per WAVEFRONT first, the read streamed twice (screen_stream.h,
 * round 6: measured, 2 x the traffic and no faster — DESIGN.md), and the persistent screen + fallback kernel takes only what
 * that leaves; A/B, tests */
#define YACRD_F_STREAM_SCREEN 65536u
/* the screen always runs in its one-item build with the second looks (sliding windows; by default only after a batch that
 * deferred more than a tenth of what it screened); tests, A/B */
#define YACRD_F_SCREEN_WIDE 2097152u
/* The long launch takes its H16 reads (129 .. 256 intervals) by read index instead of from the plan's class list, so it is
 * launched FIRST and the plan and every other register class run beside it on the engine's side stream (csrc/screen_reg.h:
 * screen_block_rows).  By default only where it pays: a long batch (the two-items build, at least 400 000
 * reads) that is at least 7/8 H16 with no read beyond 512 intervals, as far as the previous run's counts (or, without a
 * prediction, intervals / reads) say.  YACRD_F_SCREEN_DIRECT: wherever it is legal, at any batch size and without that rule; it
 * implies the long-launch build as YACRD_F_ALWAYS_DEFER | YACRD_F_SCREEN_ITEMS_2 does; tests.  YACRD_F_NO_SCREEN_DIRECT: never; A/B.
 * With YACRD_F_TIMING_FULL a direct run's yacrd_timing.plan_ms is the plan's own bracket on the side stream (it no longer
 * precedes the sweeps), and sweep_small_ms spans the screen and everything beside it. */
#define YACRD_F_SCREEN_DIRECT 8388608u
#define YACRD_F_NO_SCREEN_DIRECT 16777216u

/* the device parser's sort on its own (yacrd_amd/csrc/radix_sort.h): (key, value) pairs in host memory, sorted in place by key,
 * stable; keys must be below key_bound (it decides the number of passes); tests only */
#ifdef __cplusplus
extern "C" {
#endif
int yacrd_debug_sort_pairs(yacrd_engine *e, uint64_t *keys, uint32_t *vals, uint64_t n, uint64_t key_bound);
/* the device-side counter block of the engine's last run as it came home (csrc/device_common.h: struct Counters — class counts,
 * rejection / fallback list lengths, deferred reads): at most `bytes` of it are copied to dst; returns the block's size.
 * tools/ and tests only: the layout is not part of any ABI. */
uint64_t yacrd_debug_last_counters(const yacrd_engine *e, void *dst, uint64_t bytes);
/* the input CSR the sweeps of the engine's last call consumed, brought home from the engine's own buffers in HBM (in_off, in_iv,
 * in_len: csrc/engine_internal.h) by plain copies on the engine's stream, then a wait; no kernel runs.  It is there after a
 * successful yacrd_engine_run, yacrd_engine_submit + _collect, yacrd_stream_finish / yacrd_stream_group_finish (every engine of the
 * group: its share of the reads) and yacrd_engine[s]_ingest_overlaps[_mem] (the device parser; with several engines every engine's
 * range of the reads) — the paths on which the GPU builds or stages that CSR itself, so tests can compare it with a reference
 * interval by interval instead of through the sweep's output.  Any other call on the engine that may rewrite, move or release
 * those buffers or that sweeps the caller's device pointers (the _device and batch forms, ingest_report, classify, trim), and any
 * failed call, leaves none: then, and while a submitted batch is pending, YACRD_EINVAL is returned and nothing is written.
 * n_reads / n_intervals are always written on success; with offsets == NULL only they are (sizes first, arrays in a second
 * call).  offsets: n_reads + 1, intervals: 2 * n_intervals (start, end), lengths: n_reads.  The order of a read's intervals is
 * the build's (csrc/csr_build.h: whatever its atomics made it); a CSR staged from host arrays comes back bit for bit. */
int yacrd_debug_last_input_csr(yacrd_engine *e, uint64_t *n_reads, uint64_t *n_intervals, uint64_t *offsets, uint32_t *intervals,
                               uint32_t *lengths);
/* cross-engine copies of the N-engine device parser (yacrd_engines_ingest_overlaps) since the library was loaded, by route:
 * [0] same device (hipMemcpyAsync), [1] hipMemcpyPeerAsync, [2] staged through pinned host buffers.
 * YACRD_TEST_FORCE_PEER_COPY=peer|staged (environment, tests) forces route 1 / 2 for EVERY such copy, also between engines of
 * one device, and makes every engine gather the other engines' records instead of reading them in place: the multi-device
 * branch on a one-GPU box. */
void yacrd_debug_peer_copy_counts(uint64_t out[3]);
/* bytes the library holds right now, process-wide: [0] device memory, [1] pinned host memory.  Every allocation of
 * libyacrd_hip.so goes through the two owner types that keep these counts (csrc/engine_internal.h: DevBuf, PinBuf), except
 * yacrd_pinned_alloc's, which belongs to the caller.  Tests: what is live before an engine, stream or writer is made is live
 * again once it is closed. */
void yacrd_debug_live_bytes(uint64_t out[2]);
/* runs of this engine whose long launch went out direct (YACRD_F_SCREEN_DIRECT above) since it was created; a batch that is
 * run again (a missed prediction) counts each time */
uint64_t yacrd_debug_direct_runs(const yacrd_engine *e);
/* the reads beyond 16 384 intervals of the engine's last completed run, by the tier of the cascade that decided them (DESIGN.md
 * 3.3; every tier is exact, so the result does not say):
 *   [0] the device-wide screen (csrc/screen_big.h): the class count minus its fallback list;
 *   [1] thinned by the trimming filter and swept in LDS (csrc/sweep_big_trim.h: BT_TRIMMED);
 *   [2] entered the segmented sort (csrc/sweep_big.h);
 *   [3] handed to the exact kernel (csrc/sweep_general.h) from any of these: a reversed interval met by the filter, a read the
 *       sort's pass A found degenerate, a thinned read the LDS sweep rejected, the whole class under YACRD_F_FORCE_GENERAL.
 * A read counts once per tier it ENTERED: a thinned read that bt_sweep_kernel then rejects is under [1] and [3], a read the
 * sort sends on under [2] and [3]; [0] + [1] + [2] + (reads in [3] that entered neither [1] nor [2]) is the class count.
 * After a missed class prediction the device-wide screen goes out twice: the final pass is reported, not the sum.  A
 * batch that ran as one launch (YACRD_F_ONE_LAUNCH) has no such reads: all four are 0. */
void yacrd_debug_big_routes(const yacrd_engine *e, uint64_t out[4]);
/* the sequence editors' windows (csrc/gpu_seq_edit.hip): yacrd_engine_edit_fastq / _fasta, _mem, _gzip_mem,
 * _gzip_file, _bgzf_mem and _bgzf_file run a text of more than one window window by window, in a bounded ring of buffers; the
 * bytes written do not depend on it.
 *   window_bytes == 0            the policy: a window of 128 MiB, taken where the whole-text run finds no room (and, if the
 *                                build's measured default says so, for every text of more than one window);
 *   window_bytes == UINT64_MAX   never windows: the whole text at once, YACRD_EFALLBACK where it finds no room;
 *   any other value              rounded up to a whole 32 KiB tile; every text longer than it runs in windows (tests: 32 KiB to
 *                                4 MiB; the mover's chunk becomes min(4 MiB, the window)).
 * The BGZF-in forms (their text: the bytes the members inflate to) take a window of at least 64 KiB — the largest member — and
 * end every window where a member ends (csrc/bgzf_windows.h), so a window brings at most window_bytes of text and of
 * compressed stream, possibly no text at all.  Stays with the engine until set again.  Tests and A/B runs only. */
int yacrd_debug_seq_window(yacrd_engine *e, uint64_t window_bytes);
/* the batch size from which THIS engine takes the long-batch forms of the plan and of the follow-on step (csrc/plan_compact.h:
 * plan_kernel<4>; csrc/finish_compact.h: mark_list_kernel, deferred_list_kernel — the deferred reads two per wavefront through the
 * filtered exact sweep of csrc/sweep_filtered.h — and scan_compact_kernel<4>): batches of `min_reads` reads and more do, smaller
 * ones take the short forms.  The result does not depend on it.
 *   min_reads == 0            every batch is long;
 *   min_reads == UINT64_MAX   the default again: 400 000 reads (kPlanSmallReads), or what YACRD_SPLIT_MIN_READS said when the
 *                             library was loaded;
 * Which batches go out DIRECT (YACRD_F_SCREEN_DIRECT above) and which as one launch keep their own size rules.  Not while a
 * submitted batch is pending (YACRD_EINVAL).  Stays with the engine until set again.  Tests and A/B runs only: with
 * YACRD_F_COUNT_PREFILTERED the counter block's deferred_sorted (yacrd_debug_last_counters) then says how many of the deferred
 * reads the filtered sweep left to the whole-read sort. */
int yacrd_debug_long_min_reads(yacrd_engine *e, uint64_t min_reads);
/* the compute units the engine sizes its resident grids by (deferred_list_kernel: YK_LIST_OCC * 256 / YK_LIST_THREADS workgroups on
 * each); tests: whether a batch's list of marked reads is long enough for a workgroup's second turn */
uint64_t yacrd_debug_compute_units(const yacrd_engine *e);
/* what the engine's last sequence edit (FASTQ or FASTA, any form) ran as: [0] its windows (0: the whole text at once), [1] the
 * longest carry — the bytes a window left behind its last whole record for the next one —, [2] device bytes its two text
 * slots held (BGZF in: with the compressed slot and the member slice), [3] device bytes its two output slots held.  A failed
 * edit in windows leaves [0] = 0. */
void yacrd_debug_seq_windows(const yacrd_engine *e, uint64_t out[4]);
/* the overlap editor's windows (csrc/gpu_edit.hip): yacrd_engine_edit_overlaps, _mem, _gzip_mem and _gzip_file
 * run a text of more than one window window by window, in a bounded ring of buffers; the bytes written do not depend on it.
 * So do the _resident_ forms and an edit from the parser's mirror — the text lies in HBM already: no text slot
 * is held, window k is the mirror's bytes from k windows on — and the _bgzf_ forms: their window is at least 64 KiB, their
 * windows are the cuts of csrc/bgzf_windows.h that hold text (a window ends where a member ends), and a line may reach
 * min(chunk, the next window's bytes) into the next window.
 *   window_bytes == 0            the policy: a window of 128 MiB, taken where the whole-text run finds no room (and, if the
 *                                build's measured default says so, for every text of more than one window);
 *   window_bytes == UINT64_MAX   never windows: the whole text at once, YACRD_EFALLBACK where it finds no room;
 *   any other value              rounded up to a whole 32 KiB tile; every text longer than it runs in windows.  The mover's
 *                                chunk becomes min(4 MiB, the window): a line may reach that far into the next window, one
 *                                that reaches farther is YACRD_EFALLBACK.
 * Stays with the engine until set again.  Tests and A/B runs only. */
int yacrd_debug_edit_window(yacrd_engine *e, uint64_t window_bytes);
/* what the engine's last overlap edit (any form) ran as: [0] its windows (0: the whole text at once), [1] the farthest a line
 * that began in one window reached into the next, in bytes, [2] device bytes of its two text slots (BGZF in: with the
 * decoder's compressed slot and member slice; from the mirror: 0), [3] device bytes of its two output slots.  A failed edit in
 * windows leaves [0] = 0. */
void yacrd_debug_edit_windows(const yacrd_engine *e, uint64_t out[4]);
/* the plain-gzip decoder's chunk (csrc/gpu_gunzip_stream.hip): block starts are looked for once per `bytes` of
 * compressed payload.  0: YACRD_GUNZIP_CHUNK=<bytes> from the environment (read at every call; values under 1 024 count as
 * 1 024), else the default, 32 768; any other value is at least 1 024 (YACRD_EINVAL below it).  The text does not depend
 * on it; the spans, and so the counters, do.  Stays with the engine until set again.  Tests and A/B runs only. */
int yacrd_debug_gunzip_chunk(yacrd_engine *e, uint32_t bytes);
/* YACRD_TEST_REPORT_SEGMENT=<bytes> (environment, tests; read at every call): the size of the segments in which
 * yacrd_engine_write_report[_mem] brings the formatted text home, instead of 64 MiB (csrc/gpu_report_write.hip: kReportSegment;
 * 1 .. 2^30).  The bytes written do not depend on it: tests/test_gpu_report_write.py cuts lines at hundreds of borders. */
#ifdef __cplusplus
}
#endif

#endif
