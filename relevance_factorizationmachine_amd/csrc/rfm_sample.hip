// The exact mini-batch sampler on the device: the first B entries of
// RandomState(epoch).shuffle(arange(N)), bit-identical to rfm_sample_batches (rfm_host.cpp).
//
// NumPy's shuffle runs `for i = N-1 .. 1: j_i = random_interval(i); swap(a[i], a[j_i])`.  The
// swap partners j_i depend only on the MT19937 stream, not on the array, and given them the
// first B entries of the result follow without replaying the swaps (take j_0 = 0):
//   M[x]    = min{ i > x : j_i = x }                     (the first later step that chose x)
//   g(x)    = follow x -> M[x] while it exists           (what position x holds before step x)
//   succ(p) = min{ i > p : j_i = j_p }
//   out[p]  = g(succ(p)) if succ(p) exists, else j_p     (p < B)
// Pipeline per group of G epochs sharing one workspace (layout: SampleWs):
//   1. init     M = N (none), bucket counts = 0
//   2. draws    one wavefront per epoch: MT19937 in LDS, masked rejection window by window
//   3. count    M by atomicMin over j; bucket sizes of the positions q < B
//   4. scan     bucket sizes -> bucket starts (three launches)
//   5. scatter  the steps i with j_i < B into their buckets (unordered)
//   6. resolve  out[p] for p < B: bucket scan for succ(p), then the chase through M
#include "rfm_common.h"

namespace rfm {
namespace {

constexpr int kMtN = 624, kMtM = 397;
constexpr uint32_t kUpper = 0x80000000u, kLower = 0x7fffffffu, kMatrixA = 0x9908b0dfu;
constexpr int kScanThreads = 256, kScanItems = 4, kScanTile = kScanThreads * kScanItems;
constexpr int kWideThreads = 256;

// the workspace of G epochs: five arrays, each [G][len]
struct SampleWs {
  int32_t* j;     // [G][N] swap partner of step i (j[0] = 0)
  int32_t* m;     // [G][N] M[x], N = none
  int32_t* ent;   // [G][N] bucket entries (steps i with j_i < B); the scan's tile sums before
  int32_t* cnt;   // [G][B] bucket sizes
  int32_t* off;   // [G][B] bucket starts; after the scatter, bucket ends
};

inline int64_t ws_bytes_per_epoch(int64_t n, int64_t b) { return 12 * n + 8 * b; }

SampleWs carve(void* base, int64_t n, int64_t b, int64_t g) {
  SampleWs w;
  int32_t* p = static_cast<int32_t*>(base);
  w.j = p;
  w.m = w.j + g * n;
  w.ent = w.m + g * n;
  w.cnt = w.ent + g * n;
  w.off = w.cnt + g * b;
  return w;
}

__device__ inline uint32_t mask_for(uint32_t m) {
  m |= m >> 1;
  m |= m >> 2;
  m |= m >> 4;
  m |= m >> 8;
  m |= m >> 16;
  return m;
}

__device__ inline uint32_t temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__device__ inline uint32_t twist_word(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & kUpper) | (next & kLower);
  return far ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrixA);
}

// key[i] for i in [lo, hi) from key[i], key[i + 1] (key[0] for i = 623) and key[i + shift];
// every word of the range is read before any is written (the block is one wavefront).  The
// loads are unconditional (lanes past hi read word hi - 1) so that they issue back to back.
template <int kLo, int kHi, int kShift>
__device__ inline void twist_phase(uint32_t* key, int lane) {
  constexpr int kPer = (kHi - kLo + 63) / 64;
  uint32_t nv[kPer];
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int i = min(kLo + c * 64 + lane, kHi - 1);
    nv[c] = twist_word(key[i], key[i + 1 == kMtN ? 0 : i + 1], key[i + kShift]);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int i = kLo + c * 64 + lane;
    if (i < kHi) key[i] = nv[c];
  }
  __syncthreads();
}

// The refill of Mt19937::refill in three dependent phases: [0,227) reads the old [397,624),
// [227,454) the new [0,227), [454,624) the new [227,397) (and the new key[0] for 623).
__device__ inline void twist(uint32_t* key, int lane) {
  twist_phase<0, kMtN - kMtM, kMtM>(key, lane);
  twist_phase<kMtN - kMtM, 2 * (kMtN - kMtM), kMtM - kMtN>(key, lane);
  twist_phase<2 * (kMtN - kMtM), kMtN, kMtM - kMtN>(key, lane);
}

__global__ void __launch_bounds__(kWideThreads) sample_init_kernel(int32_t n, int32_t b, SampleWs w) {
  const int64_t e = blockIdx.y;
  int32_t* m = w.m + e * n;
  int32_t* cnt = w.cnt + e * b;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    m[i] = n;
    if (i < b) cnt[i] = 0;
  }
}

// One wavefront per epoch: j_i for i = N-1 .. 1 as NumPy's random_interval(i) draws them.
// A window holds the next (up to) 64 tempered outputs, one per lane, all masked with
// mask_for(cur).  Lane l's step is cur_l = cur - (accepts below l), in [cur - l, cur]; the lane
// is settled without knowing cur_l when the mask cannot change over that range (cur - l > mask/2)
// and v <= cur - l (accept) or v > cur (reject).  The settled lanes below the first unsettled
// lane a are taken with a ballot and a popcount prefix; lane a then has its exact cur_a and is
// drawn on its own (its mask may differ).  A window thus consumes a + 1 outputs (a >= 1: lane 0
// is always settled).
__global__ void __launch_bounds__(64) sample_draws_kernel(int32_t n, int64_t seed0, SampleWs w) {
  __shared__ uint32_t key[kMtN];
  const int lane = threadIdx.x;
  int32_t* j = w.j + int64_t(blockIdx.x) * n;
  if (lane == 0) {
    uint32_t s = uint32_t(seed0 + blockIdx.x);  // init_genrand, as Mt19937(uint32 seed)
    for (int i = 0; i < kMtN; ++i) {
      key[i] = s;
      s = 1812433253u * (s ^ (s >> 30)) + uint32_t(i) + 1u;
    }
    j[0] = 0;
  }
  __syncthreads();
  uint32_t cur = uint32_t(n - 1);
  int pos = kMtN;
  // the next full window's outputs, read while this one is settled (most windows take all 64)
  uint32_t ahead = 0u;
  bool have_ahead = false;
  // a window consumes at least one output and an output is accepted with probability > 1/2:
  // 16 N + 4096 windows are never reached (the bound only keeps the loop finite)
  const int64_t max_windows = 16 * int64_t(n) + 4096;
  for (int64_t win = 0; cur >= 1 && win < max_windows; ++win) {
    cur = __builtin_amdgcn_readfirstlane(cur);  // (wave-uniform: kept in scalar registers)
    pos = __builtin_amdgcn_readfirstlane(pos);
    if (pos >= kMtN) {
      twist(key, lane);
      pos = 0;
      have_ahead = false;
    }
    const int avail = kMtN - pos;
    const uint32_t raw = have_ahead ? ahead : (lane < avail ? temper(key[pos + lane]) : 0u);
    ahead = lane + 64 < avail ? temper(key[pos + 64 + lane]) : 0u;
    const uint32_t mask = 0xffffffffu >> __builtin_clz(cur), half = mask >> 1;  // mask_for(cur)
    const uint32_t v = raw & mask;
    const bool fixed = lane < avail && uint32_t(lane) + half < cur;  // cur - lane > half
    const bool accept = fixed && v + uint32_t(lane) <= cur;          // v <= cur - lane
    const bool settled = accept || (fixed && v > cur);
    const uint64_t unsettled = __ballot(!settled);
    const int a = unsettled ? __builtin_ctzll(unsettled) : 64;
    const uint64_t below_a = a == 64 ? ~0ull : ((1ull << a) - 1ull);
    const uint64_t acc = __ballot(accept) & below_a;
    if (accept && lane < a) {
      const int before = __popcll(acc & ((1ull << lane) - 1ull));
      j[cur - uint32_t(before)] = int32_t(v);
    }
    cur -= uint32_t(__popcll(acc));
    pos += a;
    have_ahead = a == 64;  // the next window starts at the outputs read ahead
    if (a < 64 && a < avail && cur >= 1) {  // lane a exists and holds an output
      const uint32_t va = uint32_t(__shfl(int(raw), a)) & mask_for(cur);
      if (va <= cur) {
        if (lane == 0) j[cur] = int32_t(va);
        cur -= 1;
      }
      pos += 1;
    }
  }
}

// M by atomicMin over j (a self-swap j_i = i chooses nothing earlier); bucket sizes for q < B
__global__ void __launch_bounds__(kWideThreads) sample_count_kernel(int32_t n, int32_t b, SampleWs w) {
  const int64_t e = blockIdx.y;
  const int32_t* j = w.j + e * n;
  int32_t* m = w.m + e * n;
  int32_t* cnt = w.cnt + e * b;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t q = j[i];
    if (q != int32_t(i)) atomicMin(m + q, int32_t(i));
    if (q < b) atomicAdd(cnt + q, 1);
  }
}

// exclusive scan of a block's kScanThreads values in LDS; returns the block total
__device__ inline int32_t block_exclusive_scan(int32_t& x, int32_t* sh) {
  const int t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const int32_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int32_t incl = sh[t], total = sh[kScanThreads - 1];
  __syncthreads();
  x = incl - x;
  return total;
}

// tile-local exclusive scan of cnt into off; the tile's total into ent[tile]
__global__ void __launch_bounds__(kScanThreads) sample_scan_tiles_kernel(int32_t n, int32_t b, SampleWs w) {
  __shared__ int32_t sh[kScanThreads];
  const int64_t e = blockIdx.y;
  const int32_t* cnt = w.cnt + e * b;
  int32_t* off = w.off + e * b;
  const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanItems;
  int32_t v[kScanItems], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = base + k < b ? cnt[base + k] : 0;
    sum += v[k];
  }
  int32_t x = sum;
  const int32_t total = block_exclusive_scan(x, sh);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < b) off[base + k] = x;
    x += v[k];
  }
  if (threadIdx.x == 0) w.ent[e * n + blockIdx.x] = total;
}

// exclusive scan of the tile totals of one epoch, kScanThreads at a time with a carry
__global__ void __launch_bounds__(kScanThreads) sample_scan_totals_kernel(int32_t n, int32_t n_tiles, SampleWs w) {
  __shared__ int32_t sh[kScanThreads];
  int32_t* tot = w.ent + int64_t(blockIdx.y) * n;
  int32_t carry = 0;
  for (int32_t lo = 0; lo < n_tiles; lo += kScanThreads) {
    const int32_t t = lo + int32_t(threadIdx.x);
    int32_t x = t < n_tiles ? tot[t] : 0;
    const int32_t total = block_exclusive_scan(x, sh);
    if (t < n_tiles) tot[t] = x + carry;
    carry += total;
  }
}

__global__ void __launch_bounds__(kScanThreads) sample_scan_add_kernel(int32_t n, int32_t b, SampleWs w) {
  const int64_t e = blockIdx.y;
  int32_t* off = w.off + e * b;
  const int32_t add = w.ent[e * n + blockIdx.x];
  const int64_t base = int64_t(blockIdx.x) * kScanTile;
  for (int k = threadIdx.x; k < kScanTile; k += kScanThreads)
    if (base + k < b) off[base + k] += add;
}

// steps with j_i < B into their buckets; off[q] moves from bucket q's start to its end
__global__ void __launch_bounds__(kWideThreads) sample_scatter_kernel(int32_t n, int32_t b, SampleWs w) {
  const int64_t e = blockIdx.y;
  const int32_t* j = w.j + e * n;
  int32_t* ent = w.ent + e * n;
  int32_t* off = w.off + e * b;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t q = j[i];
    if (q < b) ent[atomicAdd(off + q, 1)] = int32_t(i);
  }
}

__global__ void __launch_bounds__(kWideThreads) sample_resolve_kernel(int32_t n, int32_t b, SampleWs w,
                                                                      int32_t* out) {
  const int64_t e = blockIdx.y;
  const int32_t* j = w.j + e * n;
  const int32_t* m = w.m + e * n;
  const int32_t* ent = w.ent + e * n;
  const int32_t* off = w.off + e * b;
  int32_t* o = out + e * b;
  for (int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; p < b; p += int64_t(gridDim.x) * blockDim.x) {
    const int32_t q = j[p];
    const int32_t lo = q == 0 ? 0 : off[q - 1], hi = off[q];
    int32_t succ = n;  // none
    for (int32_t k = lo; k < hi; ++k) {
      const int32_t i = ent[k];
      if (i > int32_t(p) && i < succ) succ = i;
    }
    int32_t x = q;
    if (succ < n) {
      x = succ;
      for (int32_t s = 0; s < n; ++s) {  // M strictly increases along the chase
        const int32_t nx = m[x];
        if (nx >= n) break;
        x = nx;
      }
    }
    o[p] = x;
  }
}

}  // namespace
}  // namespace rfm

using namespace rfm;

extern "C" {

int32_t rfm_sample_batches_device_workspace(int64_t n_rows, int64_t batch_size,
                                            int64_t epochs_in_flight, int64_t* h_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_bytes, "null output");
    RFM_REQUIRE(n_rows > 0 && n_rows < (int64_t(1) << 31), "n_rows=%lld out of range",
                (long long)n_rows);
    RFM_REQUIRE(batch_size > 0, "batch_size must be positive");
    RFM_REQUIRE(batch_size <= n_rows,
                "Cannot sample %lld out of arrays with dim %lld when replace is False",
                (long long)batch_size, (long long)n_rows);
    RFM_REQUIRE(epochs_in_flight > 0 && epochs_in_flight <= (int64_t(1) << 32),
                "epochs_in_flight=%lld out of range", (long long)epochs_in_flight);
    *h_bytes = epochs_in_flight * ws_bytes_per_epoch(n_rows, batch_size);
  });
}

int32_t rfm_sample_batches_device(rfm_ctx* ctx, void* hip_stream, int64_t n_rows,
                                  int64_t batch_size, int64_t epoch_begin, int64_t n_epochs,
                                  int32_t* d_out_ids, void* d_workspace, int64_t workspace_bytes) {
  return guarded([&] {
    RFM_REQUIRE(ctx, "null ctx");
    RFM_REQUIRE(n_rows > 0 && n_rows < (int64_t(1) << 31), "n_rows=%lld out of range",
                (long long)n_rows);
    RFM_REQUIRE(batch_size > 0, "batch_size must be positive");
    RFM_REQUIRE(batch_size <= n_rows,
                "Cannot sample %lld out of arrays with dim %lld when replace is False",
                (long long)batch_size, (long long)n_rows);
    RFM_REQUIRE(epoch_begin >= 0 && epoch_begin + n_epochs <= (int64_t(1) << 32),
                "epoch seeds must fit 32 bits");
    RFM_REQUIRE(n_epochs >= 0 && (n_epochs == 0 || d_out_ids), "null output");
    if (n_epochs == 0) return;
    const int64_t per_epoch = ws_bytes_per_epoch(n_rows, batch_size);
    RFM_REQUIRE(d_workspace && workspace_bytes >= per_epoch,
                "workspace of %lld bytes is short of the %lld one epoch needs",
                (long long)workspace_bytes, (long long)per_epoch);
    // epochs per group: the workspace's, and the grid's y extent
    const int64_t group = std::min<int64_t>({n_epochs, workspace_bytes / per_epoch, 65535});
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    const int32_t n = int32_t(n_rows), b = int32_t(batch_size);
    const SampleWs w = carve(d_workspace, n_rows, batch_size, group);
    const int wide_n = capped_grid(ctx, n_rows, kWideThreads, 4, 1);
    const int wide_b = capped_grid(ctx, batch_size, kWideThreads, 4, 1);
    const int64_t n_tiles = (batch_size + kScanTile - 1) / kScanTile;
    for (int64_t e0 = 0; e0 < n_epochs; e0 += group) {
      const int g = int(std::min<int64_t>(group, n_epochs - e0));
      sample_init_kernel<<<dim3(wide_n, g), kWideThreads, 0, stream>>>(n, b, w);
      sample_draws_kernel<<<dim3(g), 64, 0, stream>>>(n, epoch_begin + e0, w);
      sample_count_kernel<<<dim3(wide_n, g), kWideThreads, 0, stream>>>(n, b, w);
      sample_scan_tiles_kernel<<<dim3(unsigned(n_tiles), g), kScanThreads, 0, stream>>>(n, b, w);
      sample_scan_totals_kernel<<<dim3(1, g), kScanThreads, 0, stream>>>(n, int32_t(n_tiles), w);
      sample_scan_add_kernel<<<dim3(unsigned(n_tiles), g), kScanThreads, 0, stream>>>(n, b, w);
      sample_scatter_kernel<<<dim3(wide_n, g), kWideThreads, 0, stream>>>(n, b, w);
      sample_resolve_kernel<<<dim3(wide_b, g), kWideThreads, 0, stream>>>(n, b, w, d_out_ids + e0 * batch_size);
      RFM_HIP_CHECK(hipGetLastError());
    }
  });
}

}  // extern "C"
