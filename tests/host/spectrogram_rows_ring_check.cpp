// Stand-alone host check of csrc/spectrogram_rows_ring.h (tests/test_spectrogram_feed_ring.py builds it with -fsanitize=address,undefined):
// the header's address functions — spec_ring_geom, spec_ring_lane_bin, spec_ring_pos — go through a CPU walk of k_spec_rows_ring's
// load / LDS / walk / chain order, workgroup by workgroup and step by step, over random rows placed by a restated dif_bin_offset; the
// result is compared bit for bit with a direct restatement of Spectrogram::process / send (spectrogram.cpp:45-75) on the bin-ordered
// rows. Every power-of-two m from 1 to n / 64 at both radices; cuts at the first frame, at the last frame, and none.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/spectrogram_rows_ring.h"

namespace {

// fft65536_dif8.h: dif_bin_offset, restated
int fold_offset(int i, int logq) {
  const int g = i & ((1 << logq) - 1), k = i >> logq;
  return ((k >> 5) << (5 + logq)) + (g << 5) + (k & 31);
}

// spectrogram_rows.h: spec_rows_i8, restated
int8_t to_i8(float v) {
  const int i = std::fabs(v) < 2147483648.0f ? (int)v : 0;
  return (int8_t)(i & 0xff);
}

struct Out {
  std::vector<float> sum, mean;
  std::vector<int8_t> rows;
};

// Spectrogram::process per frame, Spectrogram::send's arithmetic at a closing frame
Out direct(const std::vector<float>& db, int n, int nframes, int m, const std::vector<float>& sum0, int count0, const std::vector<int>& cut) {
  const int size = n / m;
  Out o{sum0, std::vector<float>(cut.size() * (size_t)size), std::vector<int8_t>(cut.size() * (size_t)size)};
  for (int b = 0; b < size; ++b) {
    float sum = sum0[(size_t)b];
    int count = count0;
    size_t k = 0;
    for (int f = 0; f < nframes; ++f) {
      float s = 0.0f;
      for (int i = 0; i < m; ++i) s += db[(size_t)f * n + (size_t)b * m + i];
      sum += s / (float)m;
      ++count;
      if (k < cut.size() && cut[k] == f) {
        const float mean = sum / (float)count;
        o.mean[k * size + b] = mean;
        o.rows[k * size + b] = to_i8(mean);
        sum = 0.0f;
        count = 0;
        ++k;
      }
    }
    o.sum[(size_t)b] = sum;
  }
  return o;
}

// k_spec_rows_ring on the CPU: 256 threads per workgroup in turn between the kernel's barriers
Out walk(const std::vector<float>& ring, int n, int nframes, int lm, int logq, const std::vector<float>& sum0, int count0, const std::vector<int>& cut) {
  const ss::SpecRingGeom g = ss::spec_ring_geom(lm, logq);
  const int size = n >> lm, nbins = 1 << g.lbins, run = 1 << g.lrun;
  const int inner = g.lrun < g.logq ? run : 1 << g.logq, outer = run / inner;
  const int nchunks = (nframes + g.chunk - 1) / g.chunk, steps = nchunks * g.nseg;
  Out o{sum0, std::vector<float>(cut.size() * (size_t)size), std::vector<int8_t>(cut.size() * (size_t)size)};
  std::vector<float> stage((size_t)ss::kSpecRingStage), means((size_t)ss::kSpecRingStage);
  for (int wg = 0; wg < (n >> g.lcol); ++wg) {
    const size_t col0 = (size_t)wg << g.lcol;
    struct Chain {
      float sum;
      int count;
      size_t k;
    };
    std::vector<Chain> chain((size_t)nbins);
    std::vector<int> bin((size_t)nbins);
    for (int lane = 0; lane < nbins; ++lane) {
      bin[(size_t)lane] = (wg << g.lbins) + ss::spec_ring_lane_bin(g, lane);
      chain[(size_t)lane] = Chain{sum0[(size_t)bin[(size_t)lane]], count0, 0};
    }
    float carry[256] = {};
    for (int step = 0; step < steps; ++step) {
      const int f0 = (step / g.nseg) * g.chunk, seg = step % g.nseg;
      const int frames = nframes - f0 < g.chunk ? nframes - f0 : g.chunk;
      for (int idx = 0; idx < 1024; ++idx) {  // the load, 16 bytes per lane, and the store as loaded
        const int fr = idx >> (g.lwidth - 2), q = idx & ((1 << (g.lwidth - 2)) - 1);
        const int f = f0 + fr < nframes ? f0 + fr : nframes - 1;
        memcpy(&stage[(size_t)4 * idx], &ring[(size_t)f * n + col0 + ((size_t)seg << g.lrun) + (size_t)(4 * q)], 16);
      }
      for (int item = 0; item < (frames << g.lbins); ++item) {  // the walk: thread item % 256
        const int fr = item >> g.lbins, lane = item & (nbins - 1);
        const float* p = stage.data() + ((size_t)fr << g.lwidth);
        int j = ss::spec_ring_lane_bin(g, lane) << g.lrun;
        float s = seg == 0 ? 0.0f : carry[item % 256];
        for (int oo = 0; oo < outer; ++oo, j += inner) {
          const float* q = p + ss::spec_ring_pos(j, g.logq);
          for (int i = 0; i < inner; ++i) s += q[i << 5];
        }
        if (seg == g.nseg - 1) means[(size_t)item] = s / (float)(1 << g.lm);
        else carry[item % 256] = s;
      }
      if (seg != g.nseg - 1) continue;
      for (int lane = 0; lane < nbins; ++lane) {  // the chains, frame by frame
        Chain& c = chain[(size_t)lane];
        for (int fr = 0; fr < frames; ++fr) {
          c.sum += means[((size_t)fr << g.lbins) + (size_t)lane];
          ++c.count;
          if (c.k < cut.size() && cut[c.k] == f0 + fr) {
            const float mean = c.sum / (float)c.count;
            o.mean[c.k * size + bin[(size_t)lane]] = mean;
            o.rows[c.k * size + bin[(size_t)lane]] = to_i8(mean);
            c.sum = 0.0f;
            c.count = 0;
            ++c.k;
          }
        }
      }
    }
    for (int lane = 0; lane < nbins; ++lane) o.sum[(size_t)bin[(size_t)lane]] = chain[(size_t)lane].sum;
  }
  return o;
}

int failures = 0;

void run_case(int logn, int nframes, int lm_lo, int lm_hi, int logq, std::mt19937& rng) {
  const int n = 1 << logn;
  std::uniform_real_distribution<float> dist(-120.0f, 10.0f);
  std::vector<float> db((size_t)nframes * n), ring(db.size());
  for (auto& v : db) v = dist(rng);
  for (int f = 0; f < nframes; ++f)
    for (int i = 0; i < n; ++i) ring[(size_t)f * n + (size_t)fold_offset(i, logq)] = db[(size_t)f * n + i];
  for (int i = 0; i < n; ++i) {  // the positions are a permutation of the row, the lane order a permutation of a block's output bins
    if (ss::spec_ring_pos(i, logq) != fold_offset(i, logq)) ++failures;
  }
  const std::vector<std::vector<int>> cut_sets = {{0, nframes / 2}, {nframes / 2, nframes - 1}, {}};
  for (int lm = lm_lo; lm <= lm_hi; ++lm) {
    const int size = n >> lm;
    const ss::SpecRingGeom g = ss::spec_ring_geom(lm, logq);
    std::vector<int> seen((size_t)1 << g.lbins, 0);
    for (int lane = 0; lane < (1 << g.lbins); ++lane) ++seen[(size_t)ss::spec_ring_lane_bin(g, lane)];
    for (int v : seen)
      if (v != 1) ++failures;
    std::vector<float> sum0((size_t)size);
    for (auto& v : sum0) v = dist(rng) * 3.0f;
    for (size_t cs = 0; cs < cut_sets.size(); ++cs) {
      std::vector<int> cut = cut_sets[cs];
      if (cut.size() == 2 && cut[0] == cut[1]) cut.pop_back();
      const int count0 = (int)cs * 5;
      const Out want = direct(db, n, nframes, 1 << lm, sum0, count0, cut), got = walk(ring, n, nframes, lm, logq, sum0, count0, cut);
      const auto same_bits = [](const std::vector<float>& a, const std::vector<float>& b) {
        return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), sizeof(float) * a.size()));
      };
      const bool same = same_bits(want.sum, got.sum) && same_bits(want.mean, got.mean) && want.rows == got.rows;
      if (!same) {
        ++failures;
        printf("FAIL n %d frames %d logq %d m %d cut set %zu\n", n, nframes, logq, 1 << lm, cs);
      }
    }
  }
  printf("n %d frames %d logq %d m %d..%d ok so far: %s\n", n, nframes, logq, 1 << lm_lo, 1 << lm_hi, failures ? "no" : "yes");
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  for (int logq = 3; logq <= 4; ++logq) {
    run_case(14, 37, 0, 8, logq, rng);   // m = 1 .. n / 64 = 256: inside a block; three steps of 16 (8) frames, the last one short
    run_case(19, 3, 8, 13, logq, rng);   // m = 256 .. n / 64 = 8192: whole blocks, and runs of more than 4096 values in two steps
  }
  if (failures) {
    printf("FAIL: %d\n", failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
