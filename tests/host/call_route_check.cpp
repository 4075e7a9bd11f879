// call_route_check.cpp — decide_call (csrc/call_route.h) without a GPU, as plain C++ under the sanitizers.
//   call_route_check               walks forms (decide_form over a configuration space: the product's choices and every switch the route
//                                  reads, each alone) and, for each, asks; asserts what the code states in prose about a route; the last
//                                  line is "forms <n> spec_forms <n> asks <n> bad <b>"
//   call_route_check --cases FILE  FILE holds lines "<case line of scripts/record_scan_form.py> | nframes n_learn device psd rel avg spec";
//                                  prints the route of each as run_batch records it (print_route), for tests/test_call_route.py to compare
//                                  with what the parent commit decided (tests/golden/call_route_parent.json)
#include <cstdint>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>

#include "scan_form_cases.h"

#include "../../rtl-sdr-scanner-cpp_amd/csrc/call_route.h"

namespace {

long g_bad = 0;
const char* g_form = "";        // what is being checked, for the first failures' lines: the form ...
const CallAsk* g_ask = nullptr;  // ... and the ask, where there is one
void describe(const char* cond) {
  printf("FAILED %s: %s", cond, g_form);
  if (g_ask) printf(" | nframes %d n_learn %d device %d psd %d rel %d avg %d spec %d", g_ask->nframes, g_ask->n_learn, g_ask->device, g_ask->psd, g_ask->rel, g_ask->avg, g_ask->spec);
  printf("\n");
}
#define EXPECT(cond)                                   \
  do {                                                 \
    if (!(cond) && ++g_bad <= 20) describe(#cond);     \
  } while (0)

// every choice the route reads, set to a value that differs from the product's
const std::vector<std::function<void(Diag&)>>& switches() {
  static const std::vector<std::function<void(Diag&)>> all = {
      [](Diag& d) { d.pipeline = false; },  [](Diag& d) { d.ring_only = false; },   [](Diag& d) { d.det_lag2 = false; },  [](Diag& d) { d.merge_65536 = false; },
      [](Diag& d) { d.merge_max_frames = 32; }, [](Diag& d) { d.dif8 = false; },    [](Diag& d) { d.plan_fused = false; }, [](Diag& d) { d.emit_on_rows = true; },
      [](Diag& d) { d.chunk_65536 = 32; },  [](Diag& d) { d.chunk_long = 0; },
  };
  return all;
}

long g_forms = 0, g_spec_forms = 0, g_asks = 0;

// the chunks of a call tile [0, nframes) once; riders are named on the first chunk only (launch_chunks takes them from the route that way)
bool chunks_tile(const CallRoute& r, int nframes) {
  if (r.chunk < 1) return false;
  int covered = 0, chunks = 0;
  for (int f0 = 0; f0 < nframes; f0 += r.chunk, ++chunks) covered += std::min(r.chunk, nframes - f0);
  const bool chunked = r.shape == CALL_ROWS256_STEP || r.shape == CALL_ROWS1024X256 || r.shape == CALL_TWO_PASS;
  return covered == nframes && (chunked || chunks == 1);
}

void check_route(const ScanForm& f, const Diag& d, unsigned flags, const CallAsk& a) {
  g_ask = &a;
  const CallRoute r = decide_call(f, d, flags, a);
  ++g_asks;
  // exactly one shape, and the one the form allows
  EXPECT(r.shape >= 0 && r.shape < kCallShapes);
  EXPECT((r.shape == CALL_DEEP) == f.deep && (r.shape == CALL_NON_STEP) == !f.step_path);
  EXPECT((r.shape == CALL_FOLD) == r.dif_call && (r.shape == CALL_MERGED) == r.merged_call);
  EXPECT(r.shape != CALL_FRAMES_8192 || f.use_fft8192);
  EXPECT(r.shape != CALL_ROWS256_STEP || f.rows256_step);
  EXPECT(r.shape != CALL_ROWS1024X256 || f.rows1024x256);
  EXPECT(r.shape != CALL_TWO_PASS || f.two_pass);
  EXPECT(r.shape != CALL_COLS_ROWS || (!f.use_fft8192 && !f.two_pass && !f.rows256_step && !f.rows1024x256));
  EXPECT(chunks_tile(r, a.nframes));
  EXPECT((r.ride_first & r.ride_second) == 0 && (r.ride_first | r.ride_second) <= 15u);  // no rider kind named twice in a call
  EXPECT(!(r.ride_second & (kRidePlan | kRideRows)));
  EXPECT(((r.ride_first & kRideRows) != 0) == r.merged_call);
  // what the comments promise of the predicates
  EXPECT(!r.dif_call || (r.ring_only && r.cull_call && r.overlap && a.n_learn == 0));
  EXPECT(!r.merged_call || (r.ring_only && r.overlap && a.nframes <= f.merge_max && !a.spec));
  EXPECT(!r.ring_only || r.db_call);
  EXPECT(r.ring_by_rows == (r.cull_call && a.n_learn == 0));
  // ... and, on the step path, the predicates as run_batch computed them before call_route.h, transcribed: ring_room as a term of
  // dif_call, db_call without it, ring_only from what place_ring answered (ring_place_at, from the window's first and last place)
  if (r.shape != CALL_DEEP && r.shape != CALL_NON_STEP) {
    const bool in_order = (flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN)) != 0;
    const bool keeps_no_plane = a.device && a.n_learn == 0 && !a.psd && !a.rel && !a.avg && !a.spec && !f.ref_nan && !(flags & SS_FLAG_KEEP_PLANES) && d.ring_only;
    const bool ring_room = a.nframes < kHistRows || kHistRows + a.nframes <= f.hist_rows;
    const bool dif_call = f.dif8 && f.cull_long && d.pipeline && keeps_no_plane && ring_room && !in_order;
    const bool db_call = f.cull_long && (!f.cull_fold_only || dif_call) && keeps_no_plane;
    const bool cull_call = f.cull_long && (!f.cull_fold_only || dif_call);
    bool ring_only_first = false, ring_only_last = false;
    if (cull_call && a.n_learn == 0) {
      const bool whole = f.cull_long;
      ring_only_first = keeps_no_plane && (a.nframes < kHistRows || ss::ring_place_at(0, f.hist_rows, a.nframes, kHistRows, whole).batch >= 0);
      ring_only_last = keeps_no_plane && (a.nframes < kHistRows || ss::ring_place_at(f.hist_rows - kHistRows, f.hist_rows, a.nframes, kHistRows, whole).batch >= 0);
    }
    const bool overlap = d.pipeline && a.n_learn == 0 && !in_order;
    const bool merged_call = f.merge && (f.rows256_step || f.rows1024x256) && overlap && ring_only_first && !a.spec && a.nframes <= f.merge_max;
    EXPECT(r.keeps_no_plane == keeps_no_plane && r.dif_call == dif_call && r.db_call == db_call && r.cull_call == cull_call);
    EXPECT(r.ring_only == ring_only_first && r.ring_only == ring_only_last);
    EXPECT(r.overlap == overlap && r.merged_call == merged_call);
    EXPECT(!dif_call || ring_only_first);              // (the failure "a fold call without a place for its rows" cannot be reached)
    EXPECT(ring_only_first || !db_call);               // (... nor the second settle_ring_db line: a call that is not ring-only is no db_call)
  }
  EXPECT(!(a.n_learn > 0 || (flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN))) || !r.overlap);
  EXPECT(!r.plan_fused || r.overlap);
  EXPECT(!r.keeps_no_plane || (a.device && !a.psd && !a.rel && !a.avg && !a.spec && a.n_learn == 0));
  EXPECT(!r.cull_call || f.cull_long);
  EXPECT(r.det_lag2 == (f.det_lag2 && r.shape != CALL_DEEP && r.shape != CALL_NON_STEP));
}

// The room for a whole batch's rows: every culling context has it for every call it accepts (so run_batch asks for no ring_room, and a
// fold call always has a place for its rows) — and then ring_place_at gives a batch region, wherever the window starts, exactly when the
// sizes say so: ring_only is a function of sizes.
void check_ring(const ScanForm& f, int max_batch) {
  g_ask = nullptr;
  if (!f.cull_long) return;
  for (int nframes = 1; nframes <= max_batch; ++nframes) {
    const bool room = nframes < kHistRows || kHistRows + nframes <= f.hist_rows;
    EXPECT(room);
    const bool sized = kHistRows + nframes <= f.hist_rows;
    for (int start : {0, (f.hist_rows - kHistRows) / 2, f.hist_rows - kHistRows})
      EXPECT((ss::ring_place_at(start, f.hist_rows, nframes, kHistRows, true).batch >= 0) == (nframes < kHistRows || sized));
    const bool every_start = nframes == 1 || (nframes >= kHistRows - 1 && nframes <= kHistRows + 1) || nframes == f.merge_max || nframes == f.merge_max + 1 || nframes == 64 ||
                             nframes == 65 || nframes == 256 || nframes == 257 || nframes == max_batch / 2 || nframes >= max_batch - 1;
    if (!every_start) continue;
    for (int start = 0; start + kHistRows <= f.hist_rows; ++start) {
      const ss::RingDecision rd = ss::ring_place_at(start, f.hist_rows, nframes, kHistRows, true);
      EXPECT((rd.batch >= 0) == (nframes < kHistRows || kHistRows + nframes <= f.hist_rows));
    }
    // (... and a buffer one row too short for the batch gives none)
    if (nframes >= kHistRows) EXPECT(ss::ring_place_at(0, kHistRows + nframes - 1, nframes, kHistRows, true).batch < 0);
  }
}

void walk_asks(const ss_config& cfg, const ScanForm& f, const Diag& d) {
  ++g_forms;
  if (f.spec_n > 0) ++g_spec_forms;
  const int mb = cfg.max_batch, chunk = call_chunk_limit(f, d) > 0 ? call_chunk_limit(f, d) : mb;
  const int frames[12] = {1, 15, 16, 17, 34, 35, 36, f.merge_max, f.merge_max + 1, chunk, chunk + 1, mb};
  check_ring(f, mb);
  for (int k = 0; k < 12; ++k) {
    const int nframes = std::min(frames[k], mb);
    for (int learn = 0; learn < 3; ++learn)
      for (int planes = 0; planes < 8; ++planes)
        for (int device = 0; device < 2; ++device)
          for (int spec = 0; spec <= (f.spec_n > 0 ? 1 : 0); ++spec) {
            CallAsk a;
            a.nframes = nframes;
            a.n_learn = learn == 0 ? 0 : learn == 1 ? 1 : nframes;
            a.device = device != 0;
            a.psd = (planes & 1) != 0;
            a.rel = (planes & 2) != 0;
            a.avg = (planes & 4) != 0;
            a.spec = spec != 0;
            check_route(f, d, cfg.flags, a);
          }
  }
}

void walk() {
  const unsigned flag_bits[5] = {SS_FLAG_KEEP_PLANES, SS_FLAG_SPECTROGRAM, SS_FLAG_NO_CULL, SS_FLAG_STREAM_ORDERED, SS_FLAG_REFERENCE_NAN};
  std::vector<Diag> diags(1);
  for (const auto& sw : switches()) {
    diags.emplace_back();
    sw(diags.back());
  }
  char name[160];
  for (int logn : {10, 13, 14, 16, 17, 18, 19, 20})
    for (int fmt : {SS_FMT_CF32, SS_FMT_CS8})
      for (int win = 0; win < 2; ++win)
        for (unsigned combo = 0; combo < 32; ++combo)
          for (int mb : {16, 1024}) {  // (1024: ss_default_config's, and large enough that the ring's 1024-row floor is not what gives a batch its room)
            unsigned flags = 0;
            for (int b = 0; b < 5; ++b)
              if (combo & (1u << b)) flags |= flag_bits[b];
            const ss_config cfg = config_of(1 << logn, (1 << logn) * 250, fmt, win != 0, flags, 21, 21, mb);
            for (size_t k = 0; k < diags.size(); ++k) {
              ScanForm f;
              char err[512] = "";
              snprintf(name, sizeof(name), "n 2^%d fmt %d window %d flags %u max_batch %d choices %zu", logn, fmt, win, flags, mb, k);
              g_form = name;
              g_ask = nullptr;
              if (decide_form(cfg, diags[k], f, err) != SS_OK) {
                EXPECT(false);
                continue;
              }
              walk_asks(cfg, f, diags[k]);
            }
          }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "--cases") == 0) {
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      const size_t bar = line.find('|');
      ss_config cfg;
      Diag diag;
      CallAsk a;
      int device, psd, rel, avg, spec;
      if (bar == std::string::npos || !parse_case(line.substr(0, bar), cfg, diag) ||
          sscanf(line.c_str() + bar + 1, "%d %d %d %d %d %d %d", &a.nframes, &a.n_learn, &device, &psd, &rel, &avg, &spec) != 7) {
        printf("bad case line: %s\n", line.c_str());
        return 2;
      }
      a.device = device, a.psd = psd, a.rel = rel, a.avg = avg, a.spec = spec;
      ScanForm f;
      char err[512] = "";
      if (decide_form(cfg, diag, f, err) != SS_OK) {
        printf("refused: %s\n", line.c_str());
        return 2;
      }
      print_route(stdout, a, decide_call(f, diag, cfg.flags, a));
    }
    return 0;
  }
  walk();
  printf("forms %ld spec_forms %ld asks %ld bad %ld\n", g_forms, g_spec_forms, g_asks, g_bad);
  return g_bad ? 1 : 0;
}
