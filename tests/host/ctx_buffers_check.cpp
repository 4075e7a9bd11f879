// ctx_buffers_check.cpp — csrc/device_buffers.h and alloc_ctx_buffers (csrc/ctx_buffers.h) against the fake HIP runtime of
// tests/host/fake_hip, under the sanitizers with the leak check on.
//   ctx_buffers_check               six forms, each allocated once with no failure and once with a failure injected at every call in turn:
//                                   whatever happens, nothing stays live, nothing is freed twice or used dead, and what() names the call
//                                   that failed. Prints "sizes <form> <bytes,...>" per form (sorted) and last "forms <n> runs <n> bad <b>"
//   ctx_buffers_check --cases FILE  "sizes=<bytes,...>" (sorted) for every case line of FILE (scripts/record_scan_form.py)
#include <algorithm>
#include <cstring>
#include <fstream>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/ctx_buffers.h"
#include "scan_form_cases.h"

namespace {

long g_bad = 0, g_runs = 0;

void expect(bool ok, const char* what, const char* form, long at) {
  if (!ok && ++g_bad <= 20) printf("FAILED %s (form %s, failure at call %ld)\n", what, form, at);
}

// one lifetime of a context's buffers; returns the number of HIP calls it made
long lifetime(const ScanForm& f, const ss_config& cfg, bool canary, long fail_at, const char* form, std::vector<size_t>* sizes) {
  fake_hip::State& st = fake_hip::state();
  st = fake_hip::State{};
  st.fail_at = fail_at;
  {
    CtxBuffers b;
    ss::hip_steps made;
    alloc_ctx_buffers(b, f, cfg, canary, made);
    if (fail_at < 0) {
      expect(made.ok() && made.what()[0] == 0, "a run without a failure is ok", form, fail_at);
      expect(b.stream && b.d_pass && b.d_stats && b.d_counts && b.d_psd2[0] && b.d_avg2[0] && b.d_mask2[0] && b.d_off4[0], "what every context has", form, fail_at);
    } else {
      expect(!made.ok() && made.error() != hipSuccess, "the failure is seen", form, fail_at);
      expect(strncmp(made.what(), st.failed.c_str(), st.failed.size()) == 0 && !st.failed.empty(), "what() names the call that failed", form, fail_at);
      expect(st.calls == fail_at + 1, "no call behind the first error", form, fail_at);
    }
    if (sizes) *sizes = st.sizes;
  }
  expect(st.live.empty(), "nothing live at the end", form, fail_at);
  expect(st.bad == 0, "nothing freed twice or used dead", form, fail_at);
  ++g_runs;
  return st.calls;
}

void print_sizes(std::vector<size_t> sizes) {
  std::sort(sizes.begin(), sizes.end());
  for (size_t k = 0; k < sizes.size(); ++k) printf("%s%zu", k ? "," : "", sizes[k]);
  printf("\n");
}

// the owners by themselves: move, reset, a step behind an error
void owners() {
  fake_hip::State& st = fake_hip::state();
  st = fake_hip::State{};
  {
    ss::device_buffer<float> a, b;
    ss::pinned_buffer<int> p;
    ss::hip_stream s;
    ss::hip_event e;
    ss::hip_steps made;
    made.alloc(a, 10).alloc(p, 4).stream(s).event(e).zero_async(a, 10, s).upload(b, std::vector<float>(7, 1.0f));
    expect(made.ok() && a && b && p && s && e, "a chain of steps", "owners", -1);
    float* was = a;
    ss::device_buffer<float> c(std::move(a));
    expect(!a && c.get() == was, "a move empties its source", "owners", -1);
    b = std::move(c);  // (frees what b held)
    expect(b.get() == was && st.live.size() == 4, "a move assignment frees what it replaces", "owners", -1);
    ss::reset_all(b, p);
    expect(!b && !p && st.live.size() == 2, "reset_all", "owners", -1);
    made.then([] { return hipErrorInvalidValue; }, "a call").alloc(a, 3);
    expect(!made.ok() && strcmp(made.what(), "a call") == 0 && !a, "nothing runs behind an error", "owners", -1);
  }
  expect(st.live.empty() && st.bad == 0, "the owners free what they hold, once", "owners", -1);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "--cases") == 0) {
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      ss_config cfg;
      Diag diag;
      ScanForm f;
      char err[512] = "";
      if (!parse_case(line, cfg, diag)) return 2;
      if (decide_form(cfg, diag, f, err) != SS_OK) {
        printf("refused\n");
        continue;
      }
      std::vector<size_t> sizes;
      lifetime(f, cfg, diag.canary, -1, line.c_str(), &sizes);
      printf("sizes=");
      print_sizes(sizes);
    }
    return g_bad ? 1 : 0;
  }
  owners();
  struct {
    const char* name;
    int n, fmt;
    unsigned flags;
    int gx, gy;
  } forms[] = {{"8192_deep", 8192, SS_FMT_CF32, 0, 21, 21},       {"8192_spectrogram", 8192, SS_FMT_CF32, SS_FLAG_SPECTROGRAM, 21, 21}, {"65536_cs8_fold", 65536, SS_FMT_CS8, 0, 21, 21},
               {"262144_merged", 262144, SS_FMT_CF32, 0, 21, 21}, {"1048576_two_pass", 1 << 20, SS_FMT_CF32, 0, 21, 21},                {"256_5x3_unfused", 256, SS_FMT_CF32, 0, 5, 3}};
  for (const auto& w : forms) {
    const ss_config cfg = config_of(w.n, w.n * 250, w.fmt, false, w.flags, w.gx, w.gy, 64);
    Diag diag;
    ScanForm f;
    char err[512] = "";
    if (decide_form(cfg, diag, f, err) != SS_OK) return 2;
    // (the forms are the ones their names say)
    expect(f.deep == (w.n == 8192) && f.dif8 == (w.fmt == SS_FMT_CS8) && f.merge == (w.n == 262144) && f.two_pass == (w.n == 1 << 20) && f.fused == (w.gx == 21), "the form", w.name, -1);
    std::vector<size_t> sizes;
    const long calls = lifetime(f, cfg, false, -1, w.name, &sizes);
    for (long at = 0; at < calls; ++at) lifetime(f, cfg, false, at, w.name, nullptr);
    printf("sizes %s ", w.name);
    print_sizes(sizes);
  }
  printf("forms %zu runs %ld bad %ld\n", sizeof(forms) / sizeof(forms[0]), g_runs, g_bad);
  return g_bad ? 1 : 0;
}
