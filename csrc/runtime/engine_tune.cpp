// Per-rank stripe engine: tuning state and the band / occupancy-cap /
// memory-policy autotune (see engine.h).
#include "stripe/engine.h"
#include "stripe/cpu_exec.h"

#include "stripe/trace.h"

#include "engine_internal.h"
#include "launch_policy.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

namespace stripe {

std::vector<int> Engine::bands() const {
  std::vector<int> b;
  for (const auto& p : prt_) b.push_back(p.band);
  return b;
}

std::vector<int> Engine::caps() const {
  std::vector<int> b;
  for (const auto& p : prt_) b.push_back(p.wgs);
  return b;
}

std::vector<int> Engine::policies() const {
  std::vector<int> b;
  for (const auto& p : prt_) b.push_back(p.nt);
  return b;
}

std::vector<int> Engine::orders() const {
  std::vector<int> b;
  for (const auto& p : prt_) b.push_back(p.order);
  return b;
}

void Engine::set_tuning(const std::vector<int>& bands, const std::vector<int>& caps,
                        const std::vector<int>& policies, const std::vector<int>& orders) {
  STRIPE_CHECK(bands.size() == prt_.size() && caps.size() == prt_.size() &&
                   (policies.empty() || policies.size() == prt_.size()) &&
                   (orders.empty() || orders.size() == prt_.size()),
               "tuning needs one entry per pass");
  for (size_t i = 0; i < prt_.size(); ++i) {
    prt_[i].band = bands[i];
    prt_[i].wgs = caps[i];
    if (!policies.empty()) prt_[i].nt = policies[i];
    if (!orders.empty()) {
      STRIPE_CHECK(orders[i] == 0 || orders[i] == 1, "task order must be 0 or 1");
      prt_[i].order = orders[i];
    }
  }
  tuned_ = true;
}

// STRIPE_SEP_ORDER=0|1 pins the separable task order (A/B runs); unset: tuned.
static int env_sep_order() {
  static const int v = [] {
    const char* e = std::getenv("STRIPE_SEP_ORDER");
    return e ? std::atoi(e) : -1;
  }();
  return v;
}

// Time each candidate band height, then each occupancy cap at the best band,
// on this rank's stripe (kernels only, no halo exchange; outputs land in the
// scratch ping-pong buffer) and keep the fastest.  The cap is tuned per box:
// the HBM-streaming cap that made a warm 16K RGB gaussian5 pass 9 % faster
// (0.311 -> 0.282 ms) reads no better than no cap on a cold clock
// (profiles/r3/headline_diag.txt), so it is measured here rather than fixed.
void Engine::autotune_bands() {
  tuned_ = true;
  if (!device() || cfg_.band > 0 || stripe().rows == 0) return;
  // 4-row bands pay off on small per-rank stripes, where a launch has too few
  // waves to hide each wave's row-step latency (8192x2048 gray sobel, one
  // rank's share of config 3 at N=4: 0.0125 ms at 4 rows vs 0.0150 at 12)
  const int cand[] = {4, 8, 12, 16, 24, 32};
  // -1: the family default (separable 2 / direct 3 workgroups per CU on
  // HBM-streaming passes, none on cache-resident ones), 0: no cap
  const int caps[] = {-1, 0, 2, 3, 4};
  const bool fixed_cap = policy::nt_wgs_knob().set;  // A/B runs pin the cap
  hipEvent_t e0 = ev_[6], e1 = ev_[7];
  // Cold tuning (EngineConfig::cold): a stripe whose steps all read from HBM
  // must not be tuned on data the previous candidate left in the 256 MiB
  // Infinity Cache (round 3 reused the warm tuning for the cold scope,
  // VERDICT r3 weak #2).  Every timed launch then reads and writes the next of
  // `nrot` scratch stripe pairs, together more than twice the cache.
  constexpr int64_t kMall = 256ll << 20;
  const int64_t pair_bytes = (int64_t)buf_[0].bytes() + (int64_t)buf_[1].bytes();
  std::vector<Buffer> scratch;
  int nrot = 0;
  if (cfg_.cold && pair_bytes <= 2 * kMall) {
    nrot = (int)std::min<int64_t>(8, (2 * kMall + pair_bytes - 1) / pair_bytes + 1);
    for (int k = 0; k < 2 * nrot; ++k) {
      scratch.emplace_back(buf_[k & 1].bytes(), true);
      HIP_CHECK(hipMemsetAsync(scratch.back().data(), 0, scratch.back().bytes(), s_compute_));
    }
  }
  int rot = 0;
  // a stream of cold frames alternates two streams (bench.py's headline), so
  // one frame's kernel boundary overlaps the next frame's launch: the cold
  // candidates are timed the same way, alternating launches between the
  // compute stream and a second one
  hipStream_t s2 = nullptr;
  hipEvent_t e_fork = nullptr, e_join = nullptr;
  if (nrot > 0 && tune_streams_ > 1) {
    HIP_CHECK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&e_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&e_join, hipEventDisableTiming));
  }
  struct TuneCleanup {
    hipStream_t& s;
    hipEvent_t& a;
    hipEvent_t& b;
    ~TuneCleanup() {
      if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } tune_cleanup{s2, e_fork, e_join};
  for (size_t i = 0; i < plan_.passes.size(); ++i) {
    const Pass& p = plan_.passes[i];
    if (p.kind != PassKind::Separable && p.kind != PassKind::Direct) continue;
    // (a pass with a statistic op in its prologue is timed with the LUT block as
    // it stands -- the static table, an identity statistic -- and without its
    // histogram or all-reduce: the candidate loops differ per rank unless the
    // tune is reduced, so a collective inside them would deadlock)
    // (a branched plan: any buffer but the current one takes the scratch output;
    // its combine passes are not tuned, they launch with whatever the buffers hold)
    PassLaunch L = make_launch(i, origin(buf_[cur_], p.cin), origin(buf_[cur_ == 0 ? 1 : 0], p.cout));
    const Rows whole{0, L.rows};
    auto launch_one = [&]() {
      if (nrot == 0) {
        launch_rows(i, L, whole, s_compute_);
        return;
      }
      hipStream_t ls = (s2 && (rot & 1)) ? s2 : s_compute_;
      // the same launch on the next scratch pair (same sizes and offsets)
      const Buffer& bi = scratch[(size_t)(2 * (rot % nrot))];
      const Buffer& bo = scratch[(size_t)(2 * (rot % nrot) + 1)];
      ++rot;
      PassLaunch R = L;
      R.in = bi.data() + (L.in - L.in_base);
      R.in_base = bi.data();
      R.in_bytes = (int64_t)bi.bytes();
      R.out = bo.data() + (L.out - L.out_base);
      R.out_base = bo.data();
      R.out_bytes = (int64_t)bo.bytes();
      launch_rows(i, R, whole, ls);
    };
    // median over 5 timed bursts (each after an untimed one) of kBurst
    // back-to-back launches: the steady state of an iterated run, where one
    // launch's tail overlaps the next one's ramp (isolated launches favour
    // taller bands by ~5 % on 20-90 us kernels); bursts of a 40-300 us kernel
    // still jitter by a few percent, about the gap between bands.
    // The candidates of one stage are timed round-robin, burst by burst, so a
    // clock or thermal drift lands on all of them alike (a sequential sweep
    // handed the drift to whichever candidate came last, and processes of the
    // same job picked 12- to 32-row bands, profiles/r6/tune/).  With a tune
    // reduce set (set_tune_reduce: max over the ranks of a job), every rank
    // decides on the same numbers, so no rank runs a configuration its own
    // noise picked.
    constexpr int kBurst = 4, kReps = 5;
    struct Cand {
      int band, wgs, nt, order;
    };
    auto burst = [&](const Cand& c) {
      L.band = c.band;
      L.wgs = c.wgs;
      L.nt = c.nt;
      L.order = c.order;
      HIP_CHECK(hipEventRecord(e0, s_compute_));
      if (s2) {
        HIP_CHECK(hipEventRecord(e_fork, s_compute_));
        HIP_CHECK(hipStreamWaitEvent(s2, e_fork, 0));
      }
      for (int k = 0; k < kBurst; ++k) launch_one();
      if (s2) {
        HIP_CHECK(hipEventRecord(e_join, s2));
        HIP_CHECK(hipStreamWaitEvent(s_compute_, e_join, 0));
      }
      HIP_CHECK(hipEventRecord(e1, s_compute_));
      HIP_CHECK(hipEventSynchronize(e1));
      return elapsed(e0, e1) / kBurst;
    };
    // each timed burst follows an untimed burst of the same candidate: what a
    // burst leaves behind (dirty lines of default-policy stores, the last
    // band's tail) is then its own, not the previous candidate's (timed right
    // after another candidate, nt stores paid for the default stores' write-
    // backs and the tune picked the default policy for a share it slows)
    auto time_set = [&](const std::vector<Cand>& cs, int reps = kReps) {
      std::vector<std::vector<float>> t(cs.size());
      for (int rep = 0; rep < reps; ++rep)
        for (size_t c = 0; c < cs.size(); ++c) {
          (void)burst(cs[c]);
          t[c].push_back(burst(cs[c]));
        }
      std::vector<float> med(cs.size());
      for (size_t c = 0; c < cs.size(); ++c) {
        std::nth_element(t[c].begin(), t[c].begin() + t[c].size() / 2, t[c].end());
        med[c] = t[c][t[c].size() / 2];
        if (tune_reduce_) med[c] = tune_reduce_(med[c]);
      }
      return med;
    };
    const int nt0 = L.nt;  // the untuned policy (cold: streaming; else the size rule)
    // clock ramp: the first candidate must not be timed on an idle-clocked GPU
    {
      L.band = 0;
      L.wgs = -1;
      const auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; k < 200; ++k) {
        for (int j = 0; j < 4; ++j) launch_one();
        HIP_CHECK(hipStreamSynchronize(s_compute_));
        if (s2) HIP_CHECK(hipStreamSynchronize(s2));
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 30.0) break;
      }
    }
    // bands (family-default cap), then the two fastest again over more bursts
    std::vector<Cand> bs;
    for (int b : cand) bs.push_back({b, -1, nt0, 0});
    std::vector<float> tb = time_set(bs);
    std::vector<size_t> idx(bs.size());
    for (size_t k = 0; k < idx.size(); ++k) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return tb[x] < tb[y]; });
    const std::vector<float> t2 = time_set({bs[idx[0]], bs[idx[1]]}, 2 * kReps);
    Cand best_c = t2[1] < t2[0] ? bs[idx[1]] : bs[idx[0]];
    float best = std::min(t2[0], t2[1]);
    // a cap or another policy / order must beat the incumbent, re-timed in the
    // same round-robin, by more than the noise floor
    auto challenge = [&](const std::vector<Cand>& cs, float margin) {
      std::vector<Cand> all = {best_c};
      all.insert(all.end(), cs.begin(), cs.end());
      const std::vector<float> t = time_set(all);
      best = t[0];
      size_t win = 0;
      for (size_t k = 1; k < all.size(); ++k)
        if (t[k] < best * margin && t[k] < t[win]) win = k;
      if (win > 0) {
        best_c = all[win];
        best = t[win];
      }
    };
    if (!fixed_cap) {
      std::vector<Cand> cs;
      for (int c : caps)
        if (c >= 0) cs.push_back({best_c.band, c, nt0, 0});
      challenge(cs, 0.995f);
    }
    if (cfg_.cold) {
      // the cache-resident policy (default stores, XCD-aware order), with and
      // without the chosen cap: kept only if it beats streaming beyond the noise
      best_c.nt = 1;
      challenge({{best_c.band, best_c.wgs, 0, 0}, {best_c.band, 0, 0, 0}}, 0.995f);
    }
    // task order of a separable pass: XCD-local runs of bands in alternating
    // directions (kRuns) move ~20 % fewer L2 fill bytes (16K RGB gaussian5,
    // FETCH_SIZE 1.31x -> 1.06x of the input) but change the DRAM access
    // pattern: kept only where it times faster, at the best band or 12 rows
    // (16K RGB: 270-272 us at 12 rows vs 277 us one-task at 16, cold N=8
    // share: no gain, profiles/r5/cold/README.md)
    if (sep_order_supported(p)) {
      if (env_sep_order() >= 0) {
        best_c.order = env_sep_order() == 1 ? 1 : 0;
      } else {
        std::vector<Cand> cs = {{best_c.band, best_c.wgs, best_c.nt, 1}};
        if (best_c.band != 12) cs.push_back({12, best_c.wgs, best_c.nt, 1});
        challenge(cs, 0.985f);  // beyond the bursts' jitter
      }
    }
    const int best_band = best_c.band, best_wgs = best_c.wgs, best_nt = best_c.nt, best_order = best_c.order;
    prt_[i].band = best_band;
    prt_[i].wgs = best_wgs;
    prt_[i].nt = best_nt;
    prt_[i].order = best_order;
    STRIPE_LOG(Info, rank_, "autotune pass " << i << (cfg_.cold ? " (cold)" : "") << ": band " << best_band
                                             << " rows, occupancy cap " << best_wgs << ", policy " << best_nt
                                             << ", task order " << best_order << " (" << best * 1e3f
                                             << " us per launch)");
  }
  if (!scratch.empty()) HIP_CHECK(hipStreamSynchronize(s_compute_));  // before the scratch stripes are freed
}

}  // namespace stripe
