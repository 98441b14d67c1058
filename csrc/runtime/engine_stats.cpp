// Per-rank stripe engine: the histogram, its all-reduce over the ranks and the
// run-time tables of the statistic ops (see engine.h).
#include "stripe/engine.h"
#include "stripe/cpu_exec.h"

#include "stripe/trace.h"

#include "engine_internal.h"

#include <cstring>

namespace stripe {

namespace {
// layout of the pinned host block of a device engine
constexpr size_t kCountBytes = (size_t)kHistBins * sizeof(uint32_t);  // k_hist's table, read back
constexpr size_t kLutOff = kCountBytes;                               // a pass's LUT block on its way up
constexpr size_t kStageOff = 4096;                                    // all-reduce messages, one slot per rank
constexpr size_t kSlotBytes = (size_t)kHistBins * sizeof(uint64_t);   // 256 x 3 u64
static_assert(kLutOff + kLutBytes <= kStageOff, "host block layout");

// Block until the work queued on a device engine's compute stream is done:
// through Comm::wait (bounded by STRIPE_COMM_TIMEOUT_S) where there is a
// communicator.  An external compute stream may be the legacy default stream
// (a null handle, e.g. torch's current stream), which Engine::wait_stream and
// Comm::wait skip: the host reads what the stream wrote, so it is waited for.
void wait_compute(Comm* comm, hipStream_t s) {
  if (!s) HIP_CHECK(hipStreamSynchronize(nullptr));
  else if (comm) comm->wait(s);
  else HIP_CHECK(hipStreamSynchronize(s));
}

// The histogram's device table, the all-reduce staging (one slot per rank, where
// the communicator's buffers live) and a device engine's pinned host block.
void ensure_hist_buffers(Buffer& table, Buffer& stage, PinnedBuffer& host, bool device, int world) {
  if (stage.data()) return;
  const size_t slots = (size_t)std::max(2, world);
  if (device) {
    table = Buffer(kCountBytes, true);
    host = PinnedBuffer(kStageOff + slots * kSlotBytes);
  }
  stage = Buffer(slots * kSlotBytes, device);
  // a device Buffer is zeroed on the default stream, which the engine's
  // non-blocking streams do not wait for: that memset must not land on counts
  // or on received messages
  if (device) HIP_CHECK(hipStreamSynchronize(nullptr));
}
}  // namespace

void Engine::fill_lut_block(const Pass& p, uint8_t* l) const {
  for (int v = 0; v < 256; ++v) {
    l[v] = p.pro.has_pre ? p.pro.pre[(size_t)v] : (uint8_t)v;
    l[256 + v] = p.pro.has_post ? p.pro.post[(size_t)v] : (uint8_t)v;
    l[512 + v] = p.has_epi ? p.epi[(size_t)v] : (uint8_t)v;
  }
}

Histogram Engine::stripe_histogram(const uint8_t* org, int C) {
  const Stripe& st = stripe();
  Histogram h(C);
  if (st.rows == 0) return h;
  if (!device()) return cpu_histogram(ConstView{org, pitch(C)}, cfg_.W, C, st.rows, host_threads());
  TraceRange tr("stripe.histogram");
  ensure_hist_buffers(hist_dev_, hist_stage_, hist_host_, device(), world_);
  HistLaunch L;
  L.in = org;
  L.pitch = pitch(C);
  L.W = cfg_.W;
  L.C = C;
  L.rows = st.rows;
  for (const Buffer* b : {&buf_[0], &buf_[1], &buf_[2]})
    if (b->data() && org >= b->data() && org < b->data() + b->bytes()) {
      L.in_base = b->data();
      L.in_bytes = (int64_t)b->bytes();
    }
  L.bins = reinterpret_cast<uint32_t*>(hist_dev_.data());
  const size_t bytes = (size_t)256 * C * sizeof(uint32_t);
  HIP_CHECK(hipMemsetAsync(hist_dev_.data(), 0, kCountBytes, s_compute_));
  launch_histogram(L, s_compute_);
  HIP_CHECK(hipMemcpyAsync(hist_host_.data(), hist_dev_.data(), bytes, hipMemcpyDeviceToHost, s_compute_));
  wait_compute(comm_, s_compute_);
  const uint32_t* c32 = reinterpret_cast<const uint32_t*>(hist_host_.data());
  for (size_t i = 0; i < h.bins.size(); ++i) h.bins[i] = c32[i];
  return h;
}

// Sum of the active ranks' counts on every active rank (idle_ranks_receive: on
// every rank of the communicator).  Two groups: the counts to rank 0, the total
// back.  Ranks that are not named here post nothing, and nobody waits for them.
Histogram Engine::reduce_histogram(const Histogram& local, bool idle_ranks_receive) {
  if (!comm_ || world_ <= 1) return local;
  const int nact = part_.active;
  const int nrecv = idle_ranks_receive ? world_ : nact;  // ranks 0 .. nrecv - 1 end with the total
  if (nrecv <= 1 || rank_ >= nrecv) return local;
  TraceRange tr("stripe.hist_reduce");
  const bool dev = device();  // (the communicator's buffers live where the engine's do)
  const size_t n = local.bins.size(), bytes = n * sizeof(uint64_t);
  ensure_hist_buffers(hist_dev_, hist_stage_, hist_host_, device(), world_);
  uint8_t* wire = hist_stage_.data();                                  // what the communicator moves
  uint8_t* host = dev ? hist_host_.data() + kStageOff : wire;          // what the host reads and writes
  hipStream_t s = dev ? s_compute_ : nullptr;
  auto up = [&](size_t slot) {  // host slot -> wire
    if (dev)
      HIP_CHECK(hipMemcpyAsync(wire + slot * kSlotBytes, host + slot * kSlotBytes, bytes, hipMemcpyHostToDevice, s));
  };
  auto down = [&](size_t slot, size_t count) {  // wire slots -> host, complete on return
    if (dev) {
      HIP_CHECK(hipMemcpyAsync(host + slot * kSlotBytes, wire + slot * kSlotBytes,
                               (count - 1) * kSlotBytes + bytes, hipMemcpyDeviceToHost, s));
      wait_compute(comm_, s);
    }
  };
  Histogram total = local;
  if (rank_ == 0) {
    if (nact > 1) {
      comm_->group_start();
      for (int r = 1; r < nact; ++r) comm_->recv(wire + (size_t)r * kSlotBytes, bytes, r, s);
      comm_->group_end();
      down(1, (size_t)nact - 1);
      for (int r = 1; r < nact; ++r) {
        uint64_t part[kHistBins];
        std::memcpy(part, host + (size_t)r * kSlotBytes, bytes);
        for (size_t i = 0; i < n; ++i) total.bins[i] += part[i];
      }
    }
    std::memcpy(host, total.bins.data(), bytes);
    up(0);
    comm_->group_start();
    for (int r = 1; r < nrecv; ++r) comm_->send(wire, bytes, r, s);
    comm_->group_end();
    if (dev) wait_compute(comm_, s);  // the staging block is free again
    return total;
  }
  if (rank_ < nact) {
    std::memcpy(host, local.bins.data(), bytes);
    up(0);
    comm_->group_start();
    comm_->send(wire, bytes, 0, s);
    comm_->group_end();
  }
  comm_->group_start();
  comm_->recv(wire + kSlotBytes, bytes, 0, s);
  comm_->group_end();
  down(1, 1);
  std::memcpy(total.bins.data(), host + kSlotBytes, bytes);
  return total;
}

Histogram Engine::histogram(bool global) {
  settle_post();  // a pending ahead exchange may still write this image's halo rows
  Histogram h = stripe_histogram(origin(buf_[cur_], cur_c_), cur_c_);
  return global ? reduce_histogram(h, /*idle_ranks_receive=*/true) : h;
}

Pass Engine::prepare_stat(const Pass& p, const uint8_t* in, int pi) {
  const Histogram h = reduce_histogram(stripe_histogram(in, p.cin), /*idle_ranks_receive=*/false);
  Pass r = resolve_stat(p, h);
  if (device()) {
    // (stripe_histogram synchronised the stream: the previous upload from this block is done)
    uint8_t* l = hist_host_.data() + kLutOff;
    fill_lut_block(r, l);
    HIP_CHECK(hipMemcpyAsync(prt_[(size_t)pi].luts.data(), l, kLutBytes, hipMemcpyHostToDevice, s_compute_));
  }
  return r;
}

}  // namespace stripe
