// scan_form_check.cpp — decide_form (csrc/scan_form.h) without a GPU, as plain C++ under the sanitizers.
//   scan_form_check               walks the configuration space and asserts what the code states in prose about the form; the last line is
//                                 "configs <n> forms <n> refused <n> bad <b>"
//   scan_form_check --cases FILE  prints the form of every case line of FILE (scripts/record_scan_form.py), for tests/test_scan_form.py to
//                                 compare with what the parent commit decided (tests/golden/scan_form_parent.json)
#include <cstdint>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <random>

#include "scan_form_cases.h"

namespace {

long g_bad = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond) && ++g_bad <= 20) printf("FAILED %s: %s\n", #cond, what); \
  } while (0)

// every choice that feeds a decision, set to a value that differs from the product's
const std::vector<std::function<void(Diag&)>>& switches() {
  static const std::vector<std::function<void(Diag&)>> all = {
      [](Diag& d) { d.backend_unfused = true; }, [](Diag& d) { d.fft_generic = true; }, [](Diag& d) { d.fft_rows_r = 0; }, [](Diag& d) { d.fft_rows_r = 1; },
      [](Diag& d) { d.fft_sub = 0; },            [](Diag& d) { d.fft_sub = 1; },        [](Diag& d) { d.fft_twopass = false; }, [](Diag& d) { d.ring_only = false; },
      [](Diag& d) { d.spec_standalone = true; }, [](Diag& d) { d.emit_wide = false; },  [](Diag& d) { d.step_long = false; }, [](Diag& d) { d.deep = false; },
      [](Diag& d) { d.cull = false; },           [](Diag& d) { d.cull_65536 = false; }, [](Diag& d) { d.rows256_step = false; }, [](Diag& d) { d.rows1024x256 = false; },
      [](Diag& d) { d.det_lag2 = false; },       [](Diag& d) { d.dif8 = false; },       [](Diag& d) { d.merge_65536 = false; }, [](Diag& d) { d.merge_max_frames = 32; },
      [](Diag& d) { d.win_calc = false; },       [](Diag& d) { d.queues = 1; },         [](Diag& d) { d.queues = 3; }, [](Diag& d) { d.queues = 9; },
      [](Diag& d) { d.canary = true; },          [](Diag& d) { d.pipeline = false; },   [](Diag& d) { d.emit_on_rows = true; }, [](Diag& d) { d.plan_fused = false; },
  };
  return all;
}

long g_configs = 0, g_forms = 0, g_refused = 0;

void check_one(const ss_config& cfg, const Diag& d, const char* what) {
  ScanForm f;
  char err[512] = "";
  const int st = decide_form(cfg, d, f, err);
  ++g_forms;
  const bool fused_ok = cfg.grouping_x == 21 && cfg.grouping_y == 21 && cfg.max_batch <= 65536 && !d.backend_unfused;
  if ((cfg.flags & SS_FLAG_REFERENCE_NAN) && !fused_ok) {  // refused, and with the parent's text
    ++g_refused;
    EXPECT(st == SS_ERR_INVALID && strcmp(err, "SS_FLAG_REFERENCE_NAN needs the 21 x 21 grouping (and max_batch <= 65536)") == 0);
    return;
  }
  EXPECT(st == SS_OK && err[0] == 0);
  const int n = cfg.fft_size;
  EXPECT(f.n == n && (1 << f.logn) == n && f.fused == fused_ok);
  // the four implications that four corrective lines of ss_create used to enforce after the fact
  EXPECT(!f.rows1024x256 || f.cull_long);
  EXPECT(!(f.merge && n == 262144) || f.rows1024x256);
  EXPECT(!f.det_lag2 || f.rows256_step || f.cull_fold_only || f.rows1024x256);
  EXPECT(!f.dif8 || f.cull_long);
  // ... and the rest of what the comments promise
  EXPECT(!f.dif8 || (f.det_lag2 && f.cull_long && !f.merge));
  EXPECT(!f.cull_fold_only || (f.dif8 && n == 131072));
  EXPECT(!f.deep || (f.nq >= 2 && f.nq <= 4 && f.npsd == 2 * f.nq && f.nbuf == 2 * f.nq && f.ncnt == 3 * f.nq && f.lag == f.nq && n == 8192));
  EXPECT(f.step_path || (f.nbuf == 1 && f.npsd == 1));
  EXPECT(!(f.tw_rowsR && f.tw_sub));
  EXPECT(!f.deep || !f.det_lag2);
  EXPECT(!f.merge || f.det_lag2);
  EXPECT(f.nbuf <= 2 * kMaxQueues && f.ncnt <= 3 * kMaxQueues && f.npsd <= 2 * kMaxQueues + 1 && f.nq <= kMaxQueues);  // (the arrays of ctx_buffers.h)
  EXPECT(f.fused == (f.hist_rows > 0) && (!f.fused || f.hist_rows >= 3 * kHistRows));
  EXPECT(f.cull_long == (f.smax_rows > 0) && (!f.cull_long || f.smax_rows >= 2 * cfg.max_batch + kHistRows + 1));
  EXPECT(f.step_path == (f.order_capacity > 0));
  EXPECT(((cfg.flags & SS_FLAG_SPECTROGRAM) != 0) == (f.spec_n > 0) && (f.spec_n == 0 || f.spec_n * f.spec_m == n));
  EXPECT(f.tw8v2 == (n == 8192 || f.dif8) && f.dif8_tab == f.dif8 && f.win1024 == f.two_pass && (!f.two_pass || n == (1 << 20)));
  EXPECT(!f.x256_tile || f.tw_rowsR);
  EXPECT(!(f.cull || f.cull_long) || f.step_path);  // (launch_learning: off the step path no call forms the per-tile-column minima of the ceiling)
  EXPECT(!(cfg.flags & SS_FLAG_NO_CULL) || (!f.cull && (!f.cull_long || f.plan_all)));
}

void walk() {
  const unsigned flag_bits[5] = {SS_FLAG_KEEP_PLANES, SS_FLAG_SPECTROGRAM, SS_FLAG_NO_CULL, SS_FLAG_STREAM_ORDERED, SS_FLAG_REFERENCE_NAN};
  std::vector<Diag> diags(1);  // the product's choices, every switch alone, seeded random combinations
  for (const auto& sw : switches()) {
    diags.emplace_back();
    sw(diags.back());
  }
  std::mt19937 rng(20240611);
  for (int k = 0; k < 300; ++k) {
    diags.emplace_back();
    for (const auto& sw : switches())
      if (rng() % 4 == 0) sw(diags.back());
  }
  char what[160];
  for (int logn = 6; logn <= 20; ++logn)
    for (int fmt : {SS_FMT_CF32, SS_FMT_CS8})
      for (int win = 0; win < 2; ++win)
        for (unsigned combo = 0; combo < 32; ++combo)
          for (int grouping = 0; grouping < 2; ++grouping)
            for (int mb : {16, 64, 1024}) {
              unsigned flags = 0;
              for (int b = 0; b < 5; ++b)
                if (combo & (1u << b)) flags |= flag_bits[b];
              const ss_config cfg = config_of(1 << logn, (1 << logn) * 250, fmt, win != 0, flags, grouping ? 5 : 21, grouping ? 3 : 21, mb);
              ++g_configs;
              for (size_t k = 0; k < diags.size(); ++k) {
                snprintf(what, sizeof(what), "n 2^%d fmt %d window %d flags %u grouping %d max_batch %d choices %zu", logn, fmt, win, flags, grouping, mb, k);
                check_one(cfg, diags[k], what);
              }
            }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "--cases") == 0) {
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      ss_config cfg;
      Diag diag;
      if (!parse_case(line, cfg, diag)) {
        printf("bad case line: %s\n", line.c_str());
        return 2;
      }
      ScanForm f;
      char err[512] = "";
      const int st = decide_form(cfg, diag, f, err);
      if (st != SS_OK) printf("status=%d err=%s", st, err);
      else print_form(f);
      printf("\n");
    }
    return 0;
  }
  walk();
  printf("configs %ld forms %ld refused %ld bad %ld\n", g_configs, g_forms, g_refused, g_bad);
  return g_bad ? 1 : 0;
}
