// scan_form.h — which form of the pipeline a configuration gets, decided once and as plain C++ (no HIP include: the stand-alone check
// tests/host/scan_form_check.cpp compiles it with g++). Diag: the implementation choices. ScanForm: everything ss_create decides from the
// configuration and the choices before it allocates anything, and nothing changes afterwards (ss_ctx derives from it). decide_form: the
// decision. ctx_buffers.h allocates from the form; specscan.hip builds the tables the form names.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/specscan.h"

namespace {

// fused back end (grouping 21 x 21): frames per tile, and the ring rows kept between batches
constexpr int kFusedTF = 16;
constexpr int kHistRows = 35;  // ss::DetectTile<21, 21, kFusedTF, 256>::H
// Deep pipelining (ScanForm::deep): a call's last stage runs four launches after its first; the two queues synchronise once in
// kDeepSyncPeriod launches on the launch three back (a wait costs ~10 us of queue time: rarely, and not within the first 32
// launches of a run): everything launched more than 4 + kDeepSyncPeriod + 3 launches ago has finished.
constexpr int kDeepSpecSlots = 64;  // calls whose spectrogram partial sums may wait to be added to their container
constexpr int kDeepFoldBatch = 8;   // ... added in batches of this many calls
constexpr int kDeepSyncPeriod = 64;
constexpr int kDeepSyncPhase = 32;
constexpr int kMaxQueues = 4;  // launch queues of the deep pipelining (ScanForm::nq)
constexpr int kDeepHorizon = 2 * kMaxQueues + kDeepSyncPeriod + 2 * kMaxQueues + 1;
// What the kernel headers fix and the sizes below depend on (specscan.hip asserts that the two agree)
constexpr int kFormLiveLists = 8, kFormLiveCap = 640, kFormLiveInts = 8192 + 16 * 1024;  // detect_fused.h: kLiveLists, kLiveCap, kLiveInts
constexpr int kFormStatWords = 64 * 16;                                                  // detect_fused.h: kStatShards * kStatShardStride
constexpr int kFormHaloSegPitch = 64;                                                    // detect_fused.h: kHaloSegPitch
constexpr int kFormNanStateInts = 45;                                                    // reference_nan.h: sizeof(NanState) / sizeof(int)

// getFft — sources/utils/radio_utils.cpp:98-104
inline int get_fft(int32_t sample_rate, int32_t max_step) {
  uint32_t v = 1;
  while ((double)max_step < (double)sample_rate / v) v <<= 1;
  return (int)v;
}

// Implementation choices. The shipped library fixes them here; a build with -DSS_DIAG (libspecscan_diag.so, used by
// the A/B tests and the measurement scripts only) lets the environment override them once, at ss_create. Nothing here
// touches the device: what a choice needs of it belongs to ss_ctx.
struct Diag {
  bool backend_unfused = false;  // per-stage back-end kernels also for the 21 x 21 grouping
  bool fft_generic = false;      // radix-4 LDS kernels instead of the register-pass ones
  int fft_rows_r = -1;           // 0 never / 1 always use k_fft_rows256xR_psd for N2 = 512..4096 (-1: up to 2048)
  int fft_sub = -1;              // 0 never / 1 always split N2 > 256 rows into radix-A step + 256-point rows (-1: from 2048)
  bool fft_twopass = true;       // 2^20 points as 1024 x 1024 in two passes (SS_FFT_TWOPASS=0: 256 x 4096 in three, as until round 3)
  bool ring_only = true;         // 2^20 points, detect mode, calls shorter than the ring: no dB plane is written (SS_RING_ONLY=0: written as ever)
  bool fft_xcd_map = true;       // XCD-aware tile order in k_fft_rows256xR_psd
  bool spec_standalone = false;  // spectrogram by its own two kernels instead of inside the detect tiles
  bool pipeline = true;          // 8192 points: defer detect / emit of a call into the next calls' launches (scan_step.h)
  int fft_tw = 2;                // 8192 points: where the twiddles come from (fft8192_v2.h: 0 global, 1 pass-2 table in LDS, 2 LDS + SGPRs)
  bool fft_swz = true;           // 8192 points: 16-byte swizzled first exchange
  int prio_fft = 0, prio_other = 0;  // s_setprio of k_scan_step's roles
  std::string stamp_path;        // SS_DIAG only: dump per-workgroup start / end stamps of the 40th full k_scan_step launch here (ss_ctx::d_stamps)
  std::string route_path;        // SS_DIAG only (SS_ROUTE_RECORD=file): run_batch appends one line per call here, the ask and the route it decided (call_route.h: print_route)
  bool cull_stats = false;       // SS_DIAG only (SS_CULL_STATS=1): tiles seen / on the culling path / culled, printed when the context goes (ss_ctx::d_cull_stats)
  bool plan_nozero = false;      // SS_DIAG only (SS_PLAN_NOZERO=1): DetectArgs::cull_stats carries the sentinel 1 instead of counters
  // SS_DIAG only, deep pipelining: the input canary. The launch of call L + 1 reads the last frames of call L's input once
  // more (the halo, run_call_deep); include/specscan.h tells callers to leave every input alone until ss_sync. A checksum of
  // those frames is taken right behind launch L (the public stream waits for it: whatever the caller enqueues there after the
  // call comes later) and again right before launch L + 1; ss_sync compares the two and fails loudly when a caller has
  // refilled the buffer in between — a case the address check of run_call_deep cannot see (the same bytes under another pointer).
  // Opt-in (SS_CANARY=1): the wait puts the public stream behind every launch, which is not what one wants to time.
  // (its buffer, event and bookkeeping: ss_ctx::d_canary and the members beside it)
  bool canary = false;
  bool emit_wide = true;         // long rows (n >= 16384): several waves per frame in the emit stage
  bool no_order_table = false;   // SS_DIAG: never use a dispatch-order table
  int hint_mode = 0;             // SS_DIAG timing ablations of the list hand-over (scan_step.h); 3: plan workgroups never publish (tests/test_gpu_wait_bound.py)
  int wait_limit = 0;            // SS_DIAG (SS_WAIT_LIMIT): StepArgs::wait_limit, 0 = the product's
  int queues = 2;                // 8192 points, deep pipelining: launch queues (2 .. 4)
  bool cull_65536 = true;        // tile culling at 65536 points (SS_CULL_65536=0: every averaging tile evaluated, as the product did until session 17 of round 4; see decide_form)
  bool rows256_step = true;      // 65536 points with tile culling: the column half as a launch of its own (the plan of the call before at its front), the ROW tiles as k_scan_step's FFT role (KIND 6) with the deferred stages riding on them (SS_ROWS256_STEP=0: columns as the FFT role, rows and plan as launches of their own)
  bool win_calc = true;          // 2^20 points in two passes and 65536 points, default window: the column tiles form their Hamming taps instead of loading them (SS_WIN_CALC=0: the table as ever)
  bool emit_on_rows = false;     // SS_DIAG (SS_EMIT_ON_ROWS=1): 65536 points, the emit stage on the row launch instead of the column launch (A/B)
  int merge_max_frames = 128;    // ... calls of up to this many frames (SS_MERGE_MAX)
  bool merge_65536 = true;       // 65536 points, detect-mode calls: ONE launch per call — the column half of call k beside the row half of call k - 1 (scan_step.h KIND 7; SS_MERGE_65536=0: two launches per call, session 20's form)
  bool det_lag2 = true;          // 65536 points with tile culling: detect(k - 2) on the column launch of call k (SS_DET_LAG2=0: detect(k - 1) on the row launch, session 19's form)
  bool dif8 = true;              // 65536 points, int8 IQ, default window, calls that keep no plane: NO work buffer — the radix-8 fold in the load stage of the 8192-point transform, eight workgroups per frame, one launch per call whatever its length (scan_step.h KIND 8, fft65536_dif8.h; SS_DIF8=0: the four-step forms of round 4)
  int plan_first = 0;            // 8192 points: the first plan_first pairs of every list of the launch's tile plan on detect workgroups of their own ahead of the FFT role (SS_PLAN_FIRST=n; 0: every pair behind an FFT workgroup's frame)
  bool rows1024x256 = true;      // 262144 points (what getFft picks at 61.44 MS/s): rows through the 1024-point row tile with run maxima and ring rows — culled, no dB plane in detect mode, the 65536-point two-launch pipeline (SS_ROWS1024X256=0: round 2's path, k_fft_rows256xR_psd, every tile evaluated)
  long long abs_start = 0;       // SS_ABS_START=n: the frame counter starts at n instead of 0 at creation and after ss_reset — sessions that cross 2^30 frames (the counter's 30-bit form indexes the long transforms' run maxima) without the twenty seconds of scanning it takes to get there (tests/test_gpu_cull.py)
  bool drain_tail_event = true;  // 8192 points, deep pipelining: an event recorded behind the drain's last command on the public stream (SS_DRAIN_TAIL_EVENT=0: none, as until session 18 of round 6): the 20-step form 25.2 against 25.85 us per step, medians of eight alternating runs (s20)
  int chunk_65536 = 256;         // 65536 points with tile culling: calls of more frames go through in chunks of this many (SS_CHUNK_65536=0: in one piece)
  int chunk_long = 16;           // 2^20 points in two passes: calls of more frames go through in chunks of this many (SS_CHUNK_LONG=0: in one piece)
  bool halo_maxima = true;       // 8192 points, deep pipelining: the re-transformed halo frames leave per-column maxima, so that the tiles of a batch's first two frame tiles are tested like the others (SS_HALO_MAXIMA=0: evaluated whatever they hold, as until session 36 of round 5)
  int list_first_fold = -1;      // ... in the fold's launches: -1 = by the launch's size (launch_step), k > 0 = k - 1 pairs
  int list_first = 64;           // long transforms with tile culling: the first pairs of the plan's list go to detect workgroups of their own, dispatched ahead of the launch's FFT role (SS_LIST_FIRST=0: every pair behind an FFT workgroup's tile, as until session 19 of round 4)
  bool plan_fused = true;        // 2^20 points in two passes: the plan of call k at the front of call k + 1's column launch (SS_PLAN_FUSED=0: a launch of its own behind call k's rows, as until session 14 of round 4)
  int ablate_roles = 0;          // SS_DIAG timing ablation (garbage results): 1 = launches carry no detect role, 2 = no emit role
  bool cull = true;              // 8192 points: detect tiles that cannot hold a candidate are not evaluated (detect_fused.h)
  bool deep = true;              // 8192 points: consecutive step launches independent of each other, alternating over two queues (see ScanForm::deep)
  bool step_long = true;         // n >= 16384: the column half of the FFT as the FFT role of k_scan_step (false: one launch per stage)
  // Dispatch order of k_scan_step's work items when all three roles ride one launch: "prefix|cycle", comma-separated
  // segments of a role letter (E emit, D detect, F FFT) and a workgroup count ('*' = all that are left); the cycle repeats
  // until every item is placed, a role that has run out is skipped.
  std::string step_order = "E*|D128,F1024";
  // n >= 16384 (the FFT role is the column half, short workgroups): detect first. 65536 x 128 frames: 63.3 us per step
  // against 64.7 with the order above and 70.7 with one launch per stage; 2^20 x 16: 216.8 / 235 / 216.9 (profiles/r02/s18).
  std::string step_order_long = "E*|D*,F*";
  // one launch per call (KIND 7): the column tiles of this call first, the row tiles of the call before behind them — two rounds of
  // workgroups whose phases overlap. In turn (R1,F1) they took 45.7 us per 128-frame call against 41.0-41.7 in two runs, 26.2 against
  // 24.0 per 64-frame call (rows first: 41.0 / 26.7): profiles/r04/s35_summary.txt
  std::string step_order_merged = "E*|D*,F*,R*";
  // ... of the radix-8 fold's launch (KIND 8; the plan's few dozen workgroups always first): the fold workgroups, then the candidate
  // lists, then the listed tiles' detect workgroups. A detect workgroup lives 10-20 us, and every one dispatched ahead of the fold
  // workgroups holds up one of the launch's last round by as much: detect first (the long transforms' order above) 52.8 us per
  // 128-frame call, this order 40.3; passengers spread between the fold workgroups (F8,E2,D1 and the like) 47-52
  // (profiles/r05/s5_summary.txt, s6_summary.txt); emit ahead of the fold workgroups: 71.7 / 129.5 us per 256- / 512-frame call against
  // 69.8 / 126.5 (s9_summary.txt)
  std::string step_order_fold = "F*,P*,E*,D*";
#ifdef SS_DIAG
  void read() {
    const auto is = [](const char* name, const char* value) {
      const char* v = getenv(name);
      return v && strcmp(v, value) == 0;
    };
    const auto tri = [](const char* name) {
      const char* v = getenv(name);
      return !v ? -1 : (v[0] == '1' ? 1 : 0);
    };
    const auto num = [](const char* name, int dflt) {
      const char* v = getenv(name);
      return v ? atoi(v) : dflt;
    };
    backend_unfused = is("SS_BACKEND", "unfused");
    fft_generic = is("SS_FFT_IMPL", "generic");
    fft_rows_r = tri("SS_FFT_ROWSR");
    fft_sub = tri("SS_FFT_SUB");
    fft_twopass = tri("SS_FFT_TWOPASS") != 0;
    ring_only = tri("SS_RING_ONLY") != 0;
    fft_xcd_map = tri("SS_FFT_XCDMAP") != 0;
    spec_standalone = is("SS_SPEC_IMPL", "standalone");
    pipeline = tri("SS_PIPELINE") != 0;
    fft_tw = num("SS_FFT_TW", 2);
    fft_swz = tri("SS_FFT_SWZ") != 0;
    prio_fft = num("SS_STEP_PRIO_FFT", 0);
    prio_other = num("SS_STEP_PRIO_OTHER", 0);
    if (const char* v = getenv("SS_STEP_STAMPS")) stamp_path = v;
    if (const char* v = getenv("SS_ROUTE_RECORD")) route_path = v;
    emit_wide = tri("SS_EMIT_WIDE") != 0;
    step_long = tri("SS_STEP_LONG") != 0;
    deep = tri("SS_DEEP") != 0;
    cull = tri("SS_CULL") != 0;
    ablate_roles = num("SS_ABLATE_ROLES", 0);
    cull_65536 = tri("SS_CULL_65536") != 0;
    rows256_step = tri("SS_ROWS256_STEP") != 0;
    plan_fused = tri("SS_PLAN_FUSED") != 0;
    list_first = num("SS_LIST_FIRST", list_first);
    halo_maxima = tri("SS_HALO_MAXIMA") != 0;
    list_first_fold = getenv("SS_LIST_FIRST") ? list_first + 1 : num("SS_LIST_FIRST_FOLD", list_first_fold);
    chunk_long = num("SS_CHUNK_LONG", chunk_long);
    chunk_65536 = num("SS_CHUNK_65536", chunk_65536);
    rows1024x256 = tri("SS_ROWS1024X256") != 0;
    if (const char* v = getenv("SS_ABS_START")) abs_start = atoll(v);
    drain_tail_event = tri("SS_DRAIN_TAIL_EVENT") != 0;
    plan_first = num("SS_PLAN_FIRST", plan_first);
    det_lag2 = tri("SS_DET_LAG2") != 0;
    dif8 = tri("SS_DIF8") != 0;
    emit_on_rows = tri("SS_EMIT_ON_ROWS") == 1;
    merge_65536 = tri("SS_MERGE_65536") != 0;
    merge_max_frames = num("SS_MERGE_MAX", merge_max_frames);
    win_calc = tri("SS_WIN_CALC") != 0;
    canary = tri("SS_CANARY") == 1;
    queues = num("SS_QUEUES", queues);
    hint_mode = num("SS_HINT_MODE", 0);
    wait_limit = num("SS_WAIT_LIMIT", 0);
    no_order_table = tri("SS_ORDER_TABLE") == 0;
    plan_nozero = tri("SS_PLAN_NOZERO") == 1;
    cull_stats = !plan_nozero && tri("SS_CULL_STATS") == 1;
    if (const char* v = getenv("SS_STEP_ORDER")) step_order = step_order_long = step_order_fold = v;
    if (const char* v = getenv("SS_STEP_ORDER_MERGED")) step_order_merged = v;
  }
#else
  void read() {}
#endif
};

// What ss_create decides once. The members are documented where they are used (ss_ctx, specscan.hip); here they are in the order
// decide_form settles them.
struct ScanForm {
  int n = 0, logn = 0;
  bool fused = false;      // back end, fused path (grouping 21 x 21, max_batch <= 65536): ring and counters are double-buffered
  bool step_path = false;  // stage pipelining (scan_step.h): what a deferred stage reads rotates over several buffers
  int spec_n = 0, spec_m = 0;   // SS_FLAG_SPECTROGRAM: output bins, input bins per output bin (spectrogram.cpp:14-15)
  bool spec_in_detect = false;  // accumulated by k_detect_fused instead of the two stand-alone kernels
  bool ref_nan = false;         // SS_FLAG_REFERENCE_NAN (reference_nan.h)
  bool deep = false;            // 8192 points: deep pipelining (the long comment in ss_ctx)
  int nq = 2;                   // ... its launch queues
  bool plan_all = false;        // SS_FLAG_NO_CULL where the fold runs: the plan lists every tile untested
  bool det_lag2 = false;        // a call's detect stage waits for its plan and rides on the column launch two calls later (stage_slots.h: DET_LAG2)
  bool merge = false;           // 65536 / 262144 points, ONE launch per call for calls that keep no dB plane (stage_slots.h: MERGED; two work buffers)
  int merge_max = 128;          // the largest call (frames) that is one launch
  bool dif8 = false;            // 65536 / 131072 points, int8 IQ or CS16 with SS_FLAG_FOLD_CS16: the radix-8 / radix-16 fold (fft65536_dif8.h)
  int dif_logq = 3;             // log2 of the fold's radix: 3 (65536 points) or 4 (131072 points: sixteen residues, KIND 9)
  bool cull_fold_only = false;  // 131072 points: the culling machinery serves the fold's calls only
  int ncnt = 3, nbuf = 1, npsd = 1, lag = 1;  // buffers in rotation: counters, mask / avg planes / offsets, internal PSD planes; launches between a call's stages
  int hist_rows = 0;            // the averager ring's capacity in rows (fused)
  bool cull = false;            // tile culling, 8192 points (detect_fused.h)
  bool deep_ring_safe = false;  // more ring windows than launches up to a run's first synchronisation (the comment in ss_ctx)
  size_t order_capacity = 0;    // entries of a dispatch-order table (step_path)
  bool use_fft256 = false, use_fft8192 = false;
  bool two_pass = false;        // N = 2^20 as 1024 x 1024 (fft1024_kernels.h): two passes over the work buffer instead of three
  // which constant tables exist (specscan.hip: upload_tables)
  bool tw256 = false, tw_small = false, tw_cols = false, tw_rowsR = false, tw_sub = false, tw8k = false, tw8v2 = false;
  bool win1024 = false, wtab = false, dif8_tab = false;
  bool x256_tile = false;     // 262144 points: the row half through the 1024-point row tile (k_fft_rows1024_psd<8>) in every context, culled or not — the same bits either way
  bool rows1024x256 = false;  // 262144 points with tile culling (round 6): 256-point column tiles as k_scan_step's FFT role with the plan of the call before, detect(k - 2) and emit(k - 3); the rows as a launch of k_fft_rows1024_psd<8>
  bool cull_long = false;     // tile culling, long transforms (the comment in ss_ctx)
  bool rows256_step = false;  // 65536 points with tile culling: columns as their own launch, rows as k_scan_step's FFT role (see Diag::rows256_step)
  int smax_rows = 0;          // frames of the run-maxima ring (cull_long)
};

// SS_OK, or SS_ERR_INVALID with its text in err[512]. From the configuration (validated by the caller) and the choices only.
inline int decide_form(const ss_config& cfg, const Diag& diag, ScanForm& f, char* err) {
  f = ScanForm{};
  const int n = cfg.fft_size;
  f.n = n;
  while ((1 << f.logn) < n) ++f.logn;
  f.fused = cfg.grouping_y == 21 && cfg.grouping_x == 21 && cfg.max_batch <= 65536 && !diag.backend_unfused;
  // 8192 points (and the four-step sizes) with the fused back end: stages of consecutive calls overlap (scan_step.h), so
  // what a deferred stage reads rotates over several buffers; every other configuration uses set 0 only
  f.step_path = f.fused && !diag.fft_generic && (n == 8192 || (n >= 16384 && diag.step_long));
  if (cfg.flags & SS_FLAG_SPECTROGRAM) {
    // output size rule of the Spectrogram block: min(SPECTROGRAM_MAX_FFT, getFft(fs, SPECTROGRAM_PREFERRED_MAX_STEP)),
    // sources/radio/blocks/spectrogram.cpp:14, config.h:36-37
    f.spec_n = std::min(std::min(get_fft(cfg.sample_rate, 1000), 16384), n);
    f.spec_m = n / f.spec_n;
    // inside the detect kernel when that kernel runs and a tile's 256 bins hold whole groups of m: one partial row per
    // frame tile (a batch that starts inside a tile touches one more)
    f.spec_in_detect = f.fused && f.spec_m <= 256 && !diag.spec_standalone;
  }
  f.ref_nan = (cfg.flags & SS_FLAG_REFERENCE_NAN) != 0;
  if (f.ref_nan && !f.fused) {
    snprintf(err, 512, "SS_FLAG_REFERENCE_NAN needs the 21 x 21 grouping (and max_batch <= 65536)");
    return SS_ERR_INVALID;
  }
  f.deep = f.step_path && n == 8192 && diag.deep && !(cfg.flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN)) && cfg.max_batch >= kHistRows &&
           (!(cfg.flags & SS_FLAG_SPECTROGRAM) || f.spec_in_detect);
  f.nq = f.deep ? std::min(std::max(diag.queues, 2), kMaxQueues) : 1;
  // 65536 points with tile culling: a call's detect stage rides two calls later (det_lag2): two more rotating sets than launches in order need
  // (131072 points — what getFft picks at 20 MS/s — have the pipeline of 65536 points where the fold can run at all: int8 IQ or flagged CS16, default window)
  const bool fold_n = n == 65536 || n == 131072;
  // what det_lag2 asks besides the size and the culling flag
  const bool lag2_base = !f.deep && f.step_path && !diag.fft_generic && diag.cull_65536 && diag.cull && diag.rows256_step && diag.step_long && diag.det_lag2 && f.fused;
  // CS16 folds where the caller asks for it (SS_FLAG_FOLD_CS16: unflagged it stays bit-identical to CF32) AND the fold then runs — at
  // a fold's size fold_ok makes plan_all of SS_FLAG_NO_CULL, so dif8 below is fold_ok && lag2_base there. Everywhere else the flag
  // reaches no field of the form: fold_fmt is its only reader (tests/host/scan_form_cs16_check.cpp).
  const bool fold_fmt = cfg.in_format == SS_FMT_CS8 || cfg.in_format == SS_FMT_CU8 ||
                        (cfg.in_format == SS_FMT_CS16 && (cfg.flags & SS_FLAG_FOLD_CS16) && fold_n && lag2_base);
  const bool fold_ok = diag.dif8 && diag.emit_wide && diag.ring_only && fold_fmt && !cfg.window &&
                       !(cfg.flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN | SS_FLAG_KEEP_PLANES | SS_FLAG_SPECTROGRAM));
  const bool x256_ok = n == 262144 && diag.rows1024x256 && diag.emit_wide && diag.fft_rows_r < 0 && diag.fft_sub < 0 && !(cfg.flags & SS_FLAG_SPECTROGRAM);
  f.plan_all = (cfg.flags & SS_FLAG_NO_CULL) && fold_ok && fold_n;  // (see ss_ctx: plan_all)
  const bool no_cull = (cfg.flags & SS_FLAG_NO_CULL) && !f.plan_all;
  f.det_lag2 = lag2_base && (n == 65536 || (n == 131072 && fold_ok) || x256_ok) && !no_cull;
  f.merge = f.det_lag2 && (n == 65536 || x256_ok) && diag.merge_65536 && diag.emit_wide;  // (one launch per call: scan_step.h KIND 7 / KIND 12, whose emit role is the wide one)
  f.merge_max = std::max(1, (int)((long long)diag.merge_max_frames * 65536 / n));  // (128 frames of 65536 points, 32 of 262144: 64 MiB of work buffer either way)
  // ... and with int8 IQ and the default window no work buffer at all: the radix-8 fold (scan_step.h KIND 8). It takes every call the
  // one-launch form above would take — and longer ones — so that form is off then.
  f.dif8 = f.det_lag2 && fold_ok && fold_n;
  f.dif_logq = n == 131072 ? 4 : 3;
  f.cull_fold_only = f.dif8 && n == 131072;
  if (f.dif8) f.merge = false;
  f.lag = f.deep ? f.nq : (f.det_lag2 ? 2 : 1);
  f.ncnt = f.deep ? 3 * f.nq : (f.merge ? 8 : f.det_lag2 ? 6 : 3);
  f.nbuf = f.deep ? 2 * f.nq : (f.merge ? 6 : f.det_lag2 ? 4 : (f.step_path ? 2 : 1));
  f.npsd = f.deep ? 2 * f.nq : (f.step_path ? 2 : 1);  // (deep: written by launch L, read by launch L + nq, written again by launch L + 2 nq on the same queue)
  if (f.fused) {
    // ring capacity: at least three windows (a long batch needs a free one next to the one it reads), more when rows
    // are small, so that short batches slide for a long time before the window is moved back to the front
    // (the window slides by a batch's frames; when it reaches the end, kHistRows rows are copied back to the front:
    // 147 MB for 2^20-point rows, so long rows get at least ten windows — one copy per ~20 sixteen-frame batches)
    long long rows = (64ll << 20) / ((long long)n * 4);
    const long long min_rows = (long long)n >= 65536 ? 10 * kHistRows : 3 * kHistRows;
    if (rows < min_rows) rows = min_rows;
    if (rows > 64 * kHistRows) rows = 64 * kHistRows;
    // (round 6: long transforms on the step path get 1024 rows — 1 GiB at 262144 points, 4 GiB at 2^20: a call shorter than the window
    // slides it along the buffer, and every return to the front is a drain of the stages that still read the old place; with 350 rows
    // 32-frame calls of 262144 points drained every eighth call, 74 us each: 9.6 of their 63 us per call, profiles/r06/s7_summary.txt;
    // 16-frame calls of 2^20 points every thirteenth. HBM is what this chip has most of.)
    if (f.step_path && n >= 65536 && rows < 1024) rows = 1024;
    // (long transforms, whose rows kernel may write ALL of a batch's rows into this buffer: three batches and the averager's reach,
    // so that a batch can go back to the front of the buffer while the one before it is still to be read — ring_place.h)
    if (n >= 65536 && f.step_path && rows < 3ll * cfg.max_batch + 3 * kHistRows) rows = 3ll * cfg.max_batch + 3 * kHistRows;
    if ((f.merge || f.dif8) && rows < 4ll * (cfg.max_batch + kHistRows)) rows = 4ll * (cfg.max_batch + kHistRows);  // (two spans to protect: ring_place.h)
    f.hist_rows = (int)rows;
  }
  f.cull = f.fused && n == 8192 && !diag.fft_generic && !(cfg.flags & SS_FLAG_NO_CULL) && diag.cull;
  if (f.deep) f.deep_ring_safe = f.hist_rows / kHistRows >= kDeepSyncPhase + 8;
  if (f.step_path)
    f.order_capacity = (size_t)(cfg.max_batch + kHistRows) * (size_t)(n / 8192) + ((size_t)cfg.max_batch / kFusedTF + 2) * (size_t)(n / 256) / 2 + (size_t)cfg.max_batch + 4 +
                       (n >= 65536 ? (size_t)cfg.max_batch * (size_t)(n / 8192) + 512 : 0) +  // (one launch per call: the row tiles of the call before, the plan workgroups)
                       (size_t)kFormLiveLists * (kFormLiveCap / 2 + 1);  // (a planned detect stage without an FFT role: 256 consumers per list, + the plan workgroups)
  // the transform and its tables
  f.tw_small = (n == 1024 || n == 2048 || n == 4096) && !diag.fft_generic;
  f.tw256 = f.tw_small || n >= 16384;
  f.tw8k = n == 8192;
  f.use_fft8192 = n == 8192 && !diag.fft_generic;
  if (n >= 16384) {
    f.use_fft256 = !diag.fft_generic;
    f.two_pass = f.use_fft256 && f.logn == 20 && diag.fft_twopass && diag.fft_rows_r < 0 && diag.fft_sub < 0;
    f.tw_cols = true;  // (two passes: one block of tables for both halves, fft1024_kernels.h, in the place of the 256-point column tiles' tables)
    const int n2size = n / 256;
    if (!f.two_pass) {
      f.tw_rowsR = n2size >= 512 && n2size <= 4096 && (diag.fft_rows_r >= 0 ? diag.fft_rows_r == 1 : n2size <= 2048);  // 4096-point rows: a tie with the two-kernel form
      f.tw_sub = n2size > 256 && !f.tw_rowsR && (diag.fft_sub >= 0 ? diag.fft_sub == 1 : n2size >= 2048);
    }
  }
  f.win1024 = f.two_pass;  // the taps in the 1024-point column tiles' own order
  f.wtab = (f.two_pass || (n == 65536 && f.use_fft256)) && !cfg.window && diag.win_calc;  // the default window: Hamming taps formed in the kernel
  f.dif8_tab = f.dif8;  // the radix-8 fold: its own tables and the 8192-point transform's
  f.tw8v2 = n == 8192 || f.dif8;
  // Tile culling for long transforms: the sizes whose rows go through k_fft_rows256_psd (N2 = 256, or the radix-A step in front)
  // and the two-pass form of 2^20 points. On by default where it pays: 2^20 points. At 65536 points it takes 7 B/sample off the
  // fabric and no time off the call: the column launch gets 10 us shorter, the plan launch costs 6.5 and the ring rows 1.4
  // (57.4 against 56.9 us per 128-frame call now that detect-mode calls write no dB plane, run_batch: ring_only; 57.1 against
  // 53.4 before; 38 against 29 us per 16-frame call either way: profiles/r04/s11_summary.txt, profiles/r03/s53_summary.txt).
  f.x256_tile = n == 262144 && f.use_fft256 && f.tw_rowsR && diag.rows1024x256 && diag.fft_rows_r < 0 && diag.fft_sub < 0;
  f.rows1024x256 = f.det_lag2 && f.x256_tile;
  f.cull_long = f.step_path && f.use_fft256 && ((n == 65536 && diag.cull_65536) || (n > 65536 && f.tw_sub && !f.tw_rowsR) || f.two_pass || f.cull_fold_only || f.rows1024x256) &&
                !no_cull && diag.cull;
  // 65536 points: with the plan of call k at the front of call k + 1's column launch — which therefore is a launch of its own, the
  // row tiles taking the FFT role of k_scan_step in its place (KIND 6) — the culling pays there too (session 17 of round 4).
  f.rows256_step = f.cull_long && !f.two_pass && f.logn == 16 && diag.rows256_step && diag.step_long;  // (no emit stage ever rides on the row launch — KIND 6, whose emit role is the wide one — but under SS_EMIT_ON_ROWS)
  // (rows1024x256 => cull_long, merge at 262144 points => rows1024x256, det_lag2 => rows256_step or cull_fold_only or rows1024x256, and
  // dif8 => cull_long: each pair is decided from the same switches, which tests/host/scan_form_check.cpp asserts over the whole space)
  if (f.cull_long) {
    int rows = 64;
    // (two batches and the averager's reach: the plan of call k — which reads the maxima of its frames and of the 35 before —
    // runs beside the column tiles of call k + 1, which clear the rows of THEIR frames: k_fft_cols1024_plan)
    // (262144 points in one launch per call: the column tiles of call k clear their frames' words while the plan of call k - 2 rides on the
    // same launch: three batches)
    while (rows < ((f.merge && f.rows1024x256) ? 3 : 2) * cfg.max_batch + kHistRows + 1) rows <<= 1;
    f.smax_rows = rows;
  }
  return SS_OK;
}

}  // namespace
