// scan_form_cs16_check.cpp — what SS_FLAG_FOLD_CS16 does to decide_form (csrc/scan_form.h), without a GPU, as plain C++ under the
// sanitizers. Over the configuration space of scan_form_check.cpp (15 sizes x windows x the 32 combinations of the older flags x
// groupings x batch sizes, under the product's choices, every switch alone and seeded random combinations):
//   an unflagged CS16 form equals the CF32 form in every field (CS16 takes CF32's path: tests/test_gpu_cs16.py);
//   a flagged CS16 form equals the CS8 form in every field where CS8's dif8 is set (the fold and everything that hangs off it);
//   a flagged CS16 form equals the unflagged CS16 form everywhere else (the flag is accepted and has no effect).
// The last line is "configs <n> forms <n> folds <n> bad <b>".
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>

#include "scan_form_cases.h"

namespace {

long g_bad = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond) && ++g_bad <= 20) printf("FAILED %s: %s\n", #cond, what); \
  } while (0)

// every member of ScanForm: 13 ints, order_capacity, 29 bools
bool same_form(const ScanForm& a, const ScanForm& b) {
  return a.n == b.n && a.logn == b.logn && a.fused == b.fused && a.step_path == b.step_path && a.spec_n == b.spec_n && a.spec_m == b.spec_m &&
         a.spec_in_detect == b.spec_in_detect && a.ref_nan == b.ref_nan && a.deep == b.deep && a.nq == b.nq && a.plan_all == b.plan_all && a.det_lag2 == b.det_lag2 &&
         a.merge == b.merge && a.merge_max == b.merge_max && a.dif8 == b.dif8 && a.dif_logq == b.dif_logq && a.cull_fold_only == b.cull_fold_only && a.ncnt == b.ncnt &&
         a.nbuf == b.nbuf && a.npsd == b.npsd && a.lag == b.lag && a.hist_rows == b.hist_rows && a.cull == b.cull && a.deep_ring_safe == b.deep_ring_safe &&
         a.order_capacity == b.order_capacity && a.use_fft256 == b.use_fft256 && a.use_fft8192 == b.use_fft8192 && a.two_pass == b.two_pass && a.tw256 == b.tw256 &&
         a.tw_small == b.tw_small && a.tw_cols == b.tw_cols && a.tw_rowsR == b.tw_rowsR && a.tw_sub == b.tw_sub && a.tw8k == b.tw8k && a.tw8v2 == b.tw8v2 &&
         a.win1024 == b.win1024 && a.wtab == b.wtab && a.dif8_tab == b.dif8_tab && a.x256_tile == b.x256_tile && a.rows1024x256 == b.rows1024x256 &&
         a.cull_long == b.cull_long && a.rows256_step == b.rows256_step && a.smax_rows == b.smax_rows;
}

const std::vector<std::function<void(Diag&)>>& switches() {  // (those of scan_form_check.cpp)
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

long g_configs = 0, g_forms = 0, g_folds = 0, g_folds_product = 0;

// 0 = refused; the four forms of one configuration differ in format and flag alone
void check_one(ss_config cfg, const Diag& d, bool product, const char* what) {
  const auto form = [&](int fmt, unsigned extra, ScanForm& f) {
    ss_config c = cfg;
    c.in_format = fmt;
    c.flags |= extra;
    char err[512] = "";
    return decide_form(c, d, f, err);
  };
  ScanForm cf32, cs8, cs16, flagged, cf32_flagged, cs8_flagged;
  const int st = form(SS_FMT_CF32, 0, cf32);
  EXPECT(form(SS_FMT_CS8, 0, cs8) == st && form(SS_FMT_CS16, 0, cs16) == st && form(SS_FMT_CS16, SS_FLAG_FOLD_CS16, flagged) == st);
  EXPECT(form(SS_FMT_CF32, SS_FLAG_FOLD_CS16, cf32_flagged) == st && form(SS_FMT_CS8, SS_FLAG_FOLD_CS16, cs8_flagged) == st);  // (never refused for the flag)
  g_forms += 6;
  if (st != SS_OK) return;
  EXPECT(same_form(cs16, cf32));
  EXPECT(same_form(cf32_flagged, cf32) && same_form(cs8_flagged, cs8));  // other formats: no effect
  if (cs8.dif8) {
    ++g_folds;
    if (product) ++g_folds_product;
    EXPECT(same_form(flagged, cs8));
    EXPECT(flagged.dif8 && (cfg.fft_size == 65536 || cfg.fft_size == 131072) && !cfg.window &&
           !(cfg.flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN | SS_FLAG_KEEP_PLANES | SS_FLAG_SPECTROGRAM)));
    EXPECT(!cs16.dif8);
  } else {
    EXPECT(same_form(flagged, cs16));
  }
}

void walk() {
  const unsigned flag_bits[5] = {SS_FLAG_KEEP_PLANES, SS_FLAG_SPECTROGRAM, SS_FLAG_NO_CULL, SS_FLAG_STREAM_ORDERED, SS_FLAG_REFERENCE_NAN};
  std::vector<Diag> diags(1);
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
    for (int win = 0; win < 2; ++win)
      for (unsigned combo = 0; combo < 32; ++combo)
        for (int grouping = 0; grouping < 2; ++grouping)
          for (int mb : {16, 64, 1024}) {
            unsigned flags = 0;
            for (int b = 0; b < 5; ++b)
              if (combo & (1u << b)) flags |= flag_bits[b];
            const ss_config cfg = config_of(1 << logn, (1 << logn) * 250, SS_FMT_CF32, win != 0, flags, grouping ? 5 : 21, grouping ? 3 : 21, mb);
            ++g_configs;
            for (size_t k = 0; k < diags.size(); ++k) {
              snprintf(what, sizeof(what), "n 2^%d window %d flags %u grouping %d max_batch %d choices %zu", logn, win, flags, grouping, mb, k);
              check_one(cfg, diags[k], k == 0, what);
            }
          }
}

}  // namespace

int main() {
  static_assert(SS_FLAG_FOLD_CS16 == 32u && SS_STATE_FOLD == 16u && SS_ABI_VERSION == 3, "the ABI of the flag");
  walk();
  // under the product's choices: 2 sizes x (flags: none, NO_CULL) x 3 batch sizes, default window, 21 x 21
  if (g_folds_product != 12) {
    printf("FAILED: %ld folding configurations under the product's choices, 12 expected\n", g_folds_product);
    ++g_bad;
  }
  printf("configs %ld forms %ld folds %ld bad %ld\n", g_configs, g_forms, g_folds, g_bad);
  return g_bad ? 1 : 0;
}
