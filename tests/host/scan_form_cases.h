// What the two host checks of the scan form share: a case line of scripts/record_scan_form.py ("n sample_rate fmt window flags gx gy
// max_batch [SS_NAME=value ...]") turned into a configuration and the choices Diag::read() makes of its switches, and the form printed
// the way the recording of the parent commit printed it (tests/golden/scan_form_parent.json).
#pragma once
#ifndef SS_DIAG
#error "the checks read the switches the way the diagnostics build does: -DSS_DIAG"
#endif
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/scan_form.h"

namespace {

const float kSomeWindow[1] = {1.0f};  // (a caller's window: the decision only asks whether there is one)

inline ss_config config_of(int n, int sample_rate, int fmt, bool window, unsigned flags, int gx, int gy, int max_batch) {
  ss_config cfg{};
  cfg.abi_version = SS_ABI_VERSION;
  cfg.fft_size = n;
  cfg.sample_rate = sample_rate;
  cfg.decim = 1;
  cfg.in_format = fmt;
  cfg.window = window ? kSomeWindow : nullptr;
  cfg.grouping_x = gx;
  cfg.grouping_y = gy;
  cfg.start_level = 8.0f;
  cfg.learn_frames = 100;
  cfg.learn_ms = 2000;
  cfg.max_batch = max_batch;
  cfg.flags = flags;
  return cfg;
}

// one case line -> cfg and diag (the switches go through the environment and Diag::read(), and are taken out of it again)
inline bool parse_case(const std::string& line, ss_config& cfg, Diag& diag) {
  std::istringstream in(line);
  int n, fs, fmt, win, gx, gy, mb;
  unsigned flags;
  if (!(in >> n >> fs >> fmt >> win >> flags >> gx >> gy >> mb)) return false;
  cfg = config_of(n, fs, fmt, win != 0, flags, gx, gy, mb);
  std::vector<std::string> names;
  for (std::string sw; in >> sw;) {
    const size_t eq = sw.find('=');
    if (eq == std::string::npos) return false;
    names.push_back(sw.substr(0, eq));
    setenv(names.back().c_str(), sw.substr(eq + 1).c_str(), 1);
  }
  diag = Diag{};
  diag.read();
  for (const auto& name : names) unsetenv(name.c_str());
  return true;
}

inline void print_form(const ScanForm& c) {
  printf("status=0 n=%d logn=%d fused=%d step_path=%d deep=%d nq=%d lag=%d ncnt=%d nbuf=%d npsd=%d det_lag2=%d merge=%d merge_max=%d dif8=%d dif_logq=%d cull_fold_only=%d plan_all=%d",
         c.n, c.logn, c.fused, c.step_path, c.deep, c.nq, c.lag, c.ncnt, c.nbuf, c.npsd, c.det_lag2, c.merge, c.merge_max, c.dif8, c.dif_logq, c.cull_fold_only, c.plan_all);
  printf(" cull=%d cull_long=%d x256_tile=%d rows1024x256=%d rows256_step=%d two_pass=%d use_fft256=%d use_fft8192=%d spec_n=%d spec_m=%d spec_in_detect=%d ref_nan=%d deep_ring_safe=%d hist_rows=%d smax_rows=%d order_capacity=%zu",
         c.cull, c.cull_long, c.x256_tile, c.rows1024x256, c.rows256_step, c.two_pass, c.use_fft256, c.use_fft8192, c.spec_n, c.spec_m, c.spec_in_detect, c.ref_nan, c.deep_ring_safe, c.hist_rows, c.smax_rows, c.order_capacity);
  printf(" tw256=%d tw_small=%d tw_cols=%d tw_rowsR=%d tw_sub=%d tw8k=%d tw8v2=%d win1024=%d wtab=%d dif8_tab=%d", c.tw256, c.tw_small, c.tw_cols, c.tw_rowsR, c.tw_sub, c.tw8k, c.tw8v2, c.win1024, c.wtab, c.dif8_tab);
}

}  // namespace
