// Fold-in examples grouped on the device: what fold.fold_examples does on the host
// -- a stable sort of the examples by new row, a bincount, label / propensity, a stable sort of the
// rows by descending count -- for a log that already lies in HBM, enqueued without a host wait.
//
// One primitive, used twice: the stable grouping of n int32 keys in [0, n_bins) (a key of -1 is left
// out) into bin_ptr int64 [n_bins + 1] and perm int32, the element indices grouped by key, ascending
// within a bin: np.argsort(keys, kind="stable").
//   count   integer atomics into a histogram, equal keys of a wavefront added once
//   scan    exclusive, three launches of our own (tile sums, the tiles' offsets, the write)
//   place   every index at an atomic cursor of its bin: a bin's order is the atomics' arrival order
//   order   every bin sorted ascending, which is the one order that does not depend on the arrival:
//           bins of 2..kWaveCap by a wavefront, kWaveCap+1..kCap by a workgroup, both by counting
//           ranks in LDS; a longer bin is rebuilt by a workgroup that walks ALL keys in input order
//           and compacts its matches (no length limit, O(n) per bin, at most n / kCap such bins)
// Integer atomics only; every loop is bounded by n or n_bins; no launch depends on a value the host
// would have to read.
#include "rfm_common.h"

namespace rfm {
namespace {

constexpr int kFgBlock = 256;      // count, place, gather, scan and the per-bin launches
constexpr int kFgWaves = kFgBlock / 64;
constexpr int kWaveCap = 256;      // longest bin a wavefront orders (4 indices per lane)
constexpr int kCap = 2048;         // longest bin ordered in LDS (8 indices per lane of a workgroup)
constexpr int kLongBlock = 1024;   // the walk of a longer bin
constexpr int kLongPer = 16;       // keys per lane and turn of that walk
constexpr int kScanPer = 8;        // histogram words per lane of a scan tile
constexpr int kScanTile = kFgBlock * kScanPer;
constexpr int kPerCu = 8;          // workgroups per CU of the grid-stride launches

__device__ __forceinline__ int lane_id() { return int(threadIdx.x) & 63; }

__device__ __forceinline__ uint64_t lanes_below() { return (uint64_t(1) << lane_id()) - 1; }

// ---------------------------------------------------------------------------
// count / place: one atomic for the lanes of a wavefront that share the first valid lane's key (one
// row can hold most of a log), one each for the rest.  Called by every lane of the wavefront.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wave_count(int32_t* hist, int32_t key, bool valid) {
  const uint64_t any = __ballot(valid);
  if (!any) return;
  const int leader = __ffsll((long long)any) - 1;
  const int32_t lead_key = __shfl(key, leader);
  const bool same = valid && key == lead_key;
  const uint64_t mates = __ballot(same);
  if (same) {
    if (lane_id() == leader) atomicAdd(&hist[lead_key], int32_t(__popcll(mates)));
  } else if (valid) {
    atomicAdd(&hist[key], 1);
  }
}

// the position of this lane's element: the bin's cursor counts DOWN from its length to zero
__device__ __forceinline__ int64_t wave_place(int32_t* hist, const int64_t* bin_ptr, int32_t key, bool valid) {
  const uint64_t any = __ballot(valid);
  if (!any) return -1;
  const int leader = __ffsll((long long)any) - 1;
  const int32_t lead_key = __shfl(key, leader);
  const bool same = valid && key == lead_key;
  const uint64_t mates = __ballot(same);
  const int32_t n_mates = int32_t(__popcll(mates));
  int32_t old = 0;
  if (same) {
    if (lane_id() == leader) old = atomicSub(&hist[lead_key], n_mates);
  } else if (valid) {
    old = atomicSub(&hist[key], 1);
  }
  const int32_t lead_old = __shfl(old, leader);
  if (!valid) return -1;
  if (same) return bin_ptr[key] + (lead_old - n_mates) + int32_t(__popcll(mates & lanes_below()));
  return bin_ptr[key] + (old - 1);
}

// ---------------------------------------------------------------------------
// keys of the two uses
// ---------------------------------------------------------------------------
// by_row: key = the new-row id, or -1 where either id is out of range; status[0], [1] count those,
// status[2] (unsigned, starts at all ones = -1) is the first such example
template <class Id>
__global__ __launch_bounds__(kFgBlock) void fg_keys_ids_kernel(const Id* d_new, const Id* d_other, int64_t stride,
                                                              int64_t n, int64_t n_new, int64_t n_fixed,
                                                              int32_t* keys, int32_t* hist, int32_t* status) {
  const int64_t step = int64_t(gridDim.x) * kFgBlock;
  for (int64_t base = int64_t(blockIdx.x) * kFgBlock; base < n; base += step) {  // (uniform in the workgroup)
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    int64_t r = -1, o = -1;
    if (in) r = int64_t(d_new[i * stride]), o = int64_t(d_other[i * stride]);
    const bool bad_new = in && (r < 0 || r >= n_new), bad_other = in && (o < 0 || o >= n_fixed);
    const uint64_t m_new = __ballot(bad_new), m_other = __ballot(bad_other);
    if (m_new | m_other) {
      const uint64_t m = m_new | m_other;
      if (lane_id() == __ffsll((long long)m) - 1) {  // the lowest bad lane holds the lowest index
        if (m_new) atomicAdd(&status[0], int32_t(__popcll(m_new)));
        if (m_other) atomicAdd(&status[1], int32_t(__popcll(m_other)));
        atomicMin(reinterpret_cast<unsigned int*>(&status[2]), (unsigned int)i);
      }
    }
    const bool valid = in && !bad_new && !bad_other;
    const int32_t key = valid ? int32_t(r) : -1;
    if (in) keys[i] = key;
    wave_count(hist, key, valid);
  }
}

// order: key of row r = n - count[r], so that the longest rows come first and ties keep their order
__global__ __launch_bounds__(kFgBlock) void fg_keys_counts_kernel(const int64_t* row_ptr, int64_t n_rows, int64_t n,
                                                                 int32_t* keys, int32_t* hist) {
  const int64_t step = int64_t(gridDim.x) * kFgBlock;
  for (int64_t base = int64_t(blockIdx.x) * kFgBlock; base < n_rows; base += step) {
    const int64_t r = base + threadIdx.x;
    const bool in = r < n_rows;
    int32_t key = -1;
    if (in) keys[r] = key = int32_t(n - (row_ptr[r + 1] - row_ptr[r]));
    wave_count(hist, key, in);
  }
}

__global__ __launch_bounds__(kFgBlock) void fg_iota_kernel(int32_t* out, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * kFgBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kFgBlock)
    out[i] = int32_t(i);
}

// ---------------------------------------------------------------------------
// scan: out[j] = sum of hist[0..j) over m words, in tiles of kScanTile
// ---------------------------------------------------------------------------
// exclusive scan of one value per lane over a workgroup of NT lanes; *total: the sum.  `part` holds
// NT / 64 words; the barriers at the end make it reusable at once.
template <int NT>
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t* part, int64_t* total) {
  int64_t inc = v;
  for (int d = 1; d < 64; d *= 2) {
    const int64_t up = __shfl_up(inc, d);
    if (lane_id() >= d) inc += up;
  }
  const int wave = int(threadIdx.x) >> 6;
  if (lane_id() == 63) part[wave] = inc;
  __syncthreads();
  int64_t before = 0, all = 0;
  for (int w = 0; w < NT / 64; ++w) {
    const int64_t p = part[w];
    if (w < wave) before += p;
    all += p;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kFgBlock) void fg_tile_sums_kernel(const int32_t* hist, int64_t m, int64_t* tile_sums) {
  __shared__ int64_t part[kFgWaves];
  const int64_t first = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
  int64_t v = 0;
  for (int j = 0; j < kScanPer; ++j)
    if (first + j < m) v += hist[first + j];
  int64_t total;
  block_scan<kFgBlock>(v, part, &total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: the tiles' sums to their exclusive offsets, in place
__global__ __launch_bounds__(kLongBlock) void fg_scan_tiles_kernel(int64_t* tile_sums, int64_t n_tiles) {
  __shared__ int64_t part[kLongBlock / 64];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kLongBlock) {
    const int64_t t = base + threadIdx.x;
    const int64_t v = t < n_tiles ? tile_sums[t] : 0;
    int64_t total;
    const int64_t ex = block_scan<kLongBlock>(v, part, &total);
    if (t < n_tiles) tile_sums[t] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(kFgBlock) void fg_scan_write_kernel(const int32_t* hist, int64_t m, const int64_t* tile_offsets,
                                                                int64_t* out) {
  __shared__ int64_t part[kFgWaves];
  const int64_t first = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
  int32_t h[kScanPer];
  int64_t v = 0;
  for (int j = 0; j < kScanPer; ++j) {
    h[j] = first + j < m ? hist[first + j] : 0;
    v += h[j];
  }
  int64_t total;
  int64_t at = tile_offsets[blockIdx.x] + block_scan<kFgBlock>(v, part, &total);
  for (int j = 0; j < kScanPer; ++j) {
    if (first + j < m) out[first + j] = at;
    at += h[j];
  }
}

// ---------------------------------------------------------------------------
// place
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kFgBlock) void fg_place_kernel(const int32_t* keys, int64_t n, int32_t* hist,
                                                           const int64_t* bin_ptr, int32_t* perm) {
  const int64_t step = int64_t(gridDim.x) * kFgBlock;
  for (int64_t base = int64_t(blockIdx.x) * kFgBlock; base < n; base += step) {
    const int64_t i = base + threadIdx.x;
    const int32_t key = i < n ? keys[i] : -1;
    const int64_t at = wave_place(hist, bin_ptr, key, key >= 0);
    if (at >= 0) perm[at] = int32_t(i);
  }
}

// ---------------------------------------------------------------------------
// order each bin
// ---------------------------------------------------------------------------
// NT lanes sort `len` <= NT * PER distinct indices at perm[lo..] ascending: each lane counts, for the
// indices it holds, the smaller ones among all of the bin in LDS (the same word for every lane of a
// read: a broadcast), and stores each at its rank.  The caller puts a barrier between load and rank.
// (Reading the bin four words at a time was measured and changed nothing: the compares bound it.)
template <int NT, int PER>
struct BinSort {
  int32_t mine[PER];
  __device__ __forceinline__ void load(const int32_t* perm, int64_t lo, int32_t len, int t, int32_t* lds) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int q = t + j * NT;
      mine[j] = 0;
      if (q < len) lds[q] = mine[j] = perm[lo + q];
    }
  }
  __device__ __forceinline__ void rank_and_store(int32_t* perm, int64_t lo, int32_t len, int t, const int32_t* lds) {
    int32_t rank[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) rank[j] = 0;
    for (int q = 0; q < len; ++q) {
      const int32_t other = lds[q];
#pragma unroll
      for (int j = 0; j < PER; ++j) rank[j] += other < mine[j];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (t + j * NT < len) perm[lo + rank[j]] = mine[j];
  }
};

// lists[0], lists[1]: the number of bins of kWaveCap+1..kCap and of more than kCap, which follow as
// two lists of `list_cap` bins each
__device__ __forceinline__ int32_t* mid_list(int32_t* lists) { return lists + 4; }
__device__ __forceinline__ int32_t* long_list(int32_t* lists, int64_t list_cap) { return lists + 4 + list_cap; }

// a wavefront per bin of 2..kWaveCap; longer bins go on their list.  Every wavefront of a workgroup
// makes the same number of turns, so the barriers are met by all.
__global__ __launch_bounds__(kFgBlock) void fg_sort_wave_kernel(const int64_t* bin_ptr, int64_t n_bins, int32_t* perm,
                                                               int32_t* lists, int64_t list_cap) {
  __shared__ int32_t lds[kFgWaves][kWaveCap];
  const int wave = int(threadIdx.x) >> 6, lane = lane_id();
  const int64_t n_groups = (n_bins + kFgWaves - 1) / kFgWaves;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t b = g * kFgWaves + wave;
    int64_t lo = 0, len = 0;
    if (b < n_bins) lo = bin_ptr[b], len = bin_ptr[b + 1] - lo;
    if (len > kWaveCap && lane == 0) {
      const bool is_long = len > kCap;
      const int32_t at = atomicAdd(&lists[is_long ? 1 : 0], 1);
      if (at < list_cap) (is_long ? long_list(lists, list_cap) : mid_list(lists))[at] = int32_t(b);
    }
    const int32_t take = (len >= 2 && len <= kWaveCap) ? int32_t(len) : 0;
    BinSort<64, kWaveCap / 64> s;
    s.load(perm, lo, take, lane, lds[wave]);
    __syncthreads();
    s.rank_and_store(perm, lo, take, lane, lds[wave]);
    __syncthreads();
  }
}

// a workgroup per listed bin of kWaveCap+1..kCap
__global__ __launch_bounds__(kFgBlock) void fg_sort_block_kernel(const int64_t* bin_ptr, int32_t* perm,
                                                                const int32_t* lists, int64_t list_cap) {
  __shared__ int32_t lds[kCap];
  const int64_t n_listed = lists[0] < list_cap ? lists[0] : list_cap;
  for (int64_t q = blockIdx.x; q < n_listed; q += gridDim.x) {
    const int64_t b = lists[4 + q];
    const int64_t lo = bin_ptr[b];
    const int64_t full = bin_ptr[b + 1] - lo;
    const int32_t len = int32_t(full < kCap ? full : kCap);
    BinSort<kFgBlock, kCap / kFgBlock> s;
    s.load(perm, lo, len, int(threadIdx.x), lds);
    __syncthreads();
    s.rank_and_store(perm, lo, len, int(threadIdx.x), lds);
    __syncthreads();
  }
}

// a workgroup per listed bin of more than kCap: all keys in input order, the matches compacted
__global__ __launch_bounds__(kLongBlock) void fg_sort_long_kernel(const int32_t* keys, int64_t n_keys,
                                                                 const int64_t* bin_ptr, int32_t* perm,
                                                                 const int32_t* lists, int64_t list_cap) {
  __shared__ int64_t part[kLongBlock / 64];
  const int64_t n_listed = lists[1] < list_cap ? lists[1] : list_cap;
  for (int64_t q = blockIdx.x; q < n_listed; q += gridDim.x) {
    const int32_t b = lists[4 + list_cap + q];
    const int64_t lo = bin_ptr[b], end = bin_ptr[b + 1];
    int64_t done = 0;
    for (int64_t base = 0; base < n_keys; base += int64_t(kLongBlock) * kLongPer) {
      const int64_t first = base + int64_t(threadIdx.x) * kLongPer;
      uint32_t hits = 0;  // bit j: key first + j is the bin's
      if (first + kLongPer <= n_keys) {  // (keys is 16-byte aligned, first a multiple of kLongPer)
        const int4* four = reinterpret_cast<const int4*>(keys + first);
#pragma unroll
        for (int c = 0; c < kLongPer / 4; ++c) {
          const int4 v = four[c];
          hits |= uint32_t((v.x == b) | (v.y == b) << 1 | (v.z == b) << 2 | (v.w == b) << 3) << (4 * c);
        }
      } else {
        for (int j = 0; j < kLongPer; ++j)
          if (first + j < n_keys && keys[first + j] == b) hits |= uint32_t(1) << j;
      }
      int64_t total;
      int64_t at = lo + done + block_scan<kLongBlock>(int64_t(__popc(hits)), part, &total);
      for (; hits && at < end; hits &= hits - 1)  // (at < end: the histogram counted them)
        perm[at++] = int32_t(first + __ffs(hits) - 1);
      done += total;
    }
  }
}

// ---------------------------------------------------------------------------
// the examples behind by_row: the other column and label / propensity, an IEEE double quotient
// ---------------------------------------------------------------------------
template <class Id>
__global__ __launch_bounds__(kFgBlock) void fg_gather_kernel(const int32_t* perm, const int64_t* row_ptr, int64_t n_new,
                                                            int64_t n, const Id* d_other, int64_t stride,
                                                            const double* labels, const double* pscores,
                                                            int32_t* ids, double* ry) {
  const int64_t kept = row_ptr[n_new] < n ? row_ptr[n_new] : n;
  for (int64_t p = int64_t(blockIdx.x) * kFgBlock + threadIdx.x; p < kept; p += int64_t(gridDim.x) * kFgBlock) {
    const int64_t i = perm[p];
    ids[p] = int32_t(d_other[i * stride]);
    ry[p] = labels[i] / pscores[i];
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int64_t kLimit = int64_t(1) << 31;

inline int64_t align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// the workspace of rfm_fold_group: offsets in bytes, every part 16-byte aligned
struct Workspace {
  int64_t keys, perm, hist, keys2, bin_ptr2, tiles, lists, bytes;
  int64_t hist_words, list_cap;
  Workspace(int64_t n, int64_t n_new) {
    hist_words = std::max(n_new, n + 1) + 1;       // bins + 1 of the larger pass
    list_cap = std::max(n, n_new) / (kWaveCap + 1) + 1;  // bins of more than kWaveCap among that many elements
    int64_t at = 0;
    auto take = [&](int64_t b) { const int64_t was = at; at += align16(b); return was; };
    keys = take(n * 4);
    perm = take(n * 4);
    hist = take(hist_words * 4);
    keys2 = take(n_new * 4);
    bin_ptr2 = take((n + 2) * 8);
    tiles = take(((hist_words + kScanTile - 1) / kScanTile + 1) * 8);
    lists = take((4 + 2 * list_cap) * 4);
    bytes = std::max<int64_t>(at, 16);
  }
};

struct Grids {
  int elements, per_bin, mid, lng;
};

inline Grids grids_for(const rfm_ctx* ctx, int64_t n, int64_t n_bins) {
  Grids g;
  g.elements = capped_grid(ctx, n, kFgBlock, kPerCu, 1);
  g.per_bin = capped_grid(ctx, n_bins, kFgWaves, kPerCu, 1);
  g.mid = capped_grid(ctx, n / (kWaveCap + 1), 1, kPerCu, 0);  // no bin of that length among fewer elements
  g.lng = capped_grid(ctx, n / (kCap + 1), 1, kPerCu, 0);
  return g;
}

// the primitive: keys [n] (already counted into hist [n_bins + 1], whose last word is zero) to
// bin_ptr [n_bins + 1] and perm
void group_counted(rfm_ctx* ctx, const int32_t* keys, int64_t n, int64_t n_bins, int32_t* hist, int64_t* bin_ptr,
                   int32_t* perm, int64_t* tiles, int32_t* lists, int64_t list_cap) {
  hipStream_t st = ctx->stream;
  const int64_t m = n_bins + 1;
  const int64_t n_tiles = (m + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(fg_tile_sums_kernel, dim3(unsigned(n_tiles)), dim3(kFgBlock), 0, st, hist, m, tiles);
  hipLaunchKernelGGL(fg_scan_tiles_kernel, dim3(1), dim3(kLongBlock), 0, st, tiles, n_tiles);
  hipLaunchKernelGGL(fg_scan_write_kernel, dim3(unsigned(n_tiles)), dim3(kFgBlock), 0, st, hist, m, tiles, bin_ptr);
  const Grids g = grids_for(ctx, n, n_bins);
  hipLaunchKernelGGL(fg_place_kernel, dim3(g.elements), dim3(kFgBlock), 0, st, keys, n, hist, bin_ptr, perm);
  RFM_HIP_CHECK(hipMemsetAsync(lists, 0, 16, st));
  hipLaunchKernelGGL(fg_sort_wave_kernel, dim3(g.per_bin), dim3(kFgBlock), 0, st, bin_ptr, n_bins, perm, lists, list_cap);
  if (g.mid)
    hipLaunchKernelGGL(fg_sort_block_kernel, dim3(g.mid), dim3(kFgBlock), 0, st, bin_ptr, perm, lists, list_cap);
  if (g.lng)
    hipLaunchKernelGGL(fg_sort_long_kernel, dim3(g.lng), dim3(kLongBlock), 0, st, keys, n, bin_ptr, perm, lists, list_cap);
  RFM_HIP_CHECK(hipGetLastError());
}

template <class Id>
void fold_group(rfm_ctx* ctx, const void* d_new, const void* d_other, int64_t stride, const double* d_labels,
                const double* d_pscores, int64_t n, int64_t n_new, int64_t n_fixed, char* ws, int64_t* d_row_ptr,
                int32_t* d_ids, double* d_ry, int32_t* d_order, int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const Workspace w(n, n_new);
  int32_t* keys = reinterpret_cast<int32_t*>(ws + w.keys);
  int32_t* perm = reinterpret_cast<int32_t*>(ws + w.perm);
  int32_t* hist = reinterpret_cast<int32_t*>(ws + w.hist);
  int32_t* keys2 = reinterpret_cast<int32_t*>(ws + w.keys2);
  int64_t* bin_ptr2 = reinterpret_cast<int64_t*>(ws + w.bin_ptr2);
  int64_t* tiles = reinterpret_cast<int64_t*>(ws + w.tiles);
  int32_t* lists = reinterpret_cast<int32_t*>(ws + w.lists);
  const Id* col_new = static_cast<const Id*>(d_new);
  const Id* col_other = static_cast<const Id*>(d_other);
  // by_row: the examples grouped by new row; its bin_ptr is row_ptr
  const Grids g1 = grids_for(ctx, n, n_new);
  RFM_HIP_CHECK(hipMemsetAsync(hist, 0, size_t(n_new + 1) * 4, st));
  hipLaunchKernelGGL(fg_keys_ids_kernel<Id>, dim3(g1.elements), dim3(kFgBlock), 0, st, col_new, col_other, stride, n, n_new,
                     n_fixed, keys, hist, d_status);
  group_counted(ctx, keys, n, n_new, hist, d_row_ptr, perm, tiles, lists, w.list_cap);
  hipLaunchKernelGGL(fg_gather_kernel<Id>, dim3(g1.elements), dim3(kFgBlock), 0, st, perm, d_row_ptr, n_new, n, col_other,
                     stride, d_labels, d_pscores, d_ids, d_ry);
  // order: the rows grouped by n - count, n + 1 bins
  const Grids g2 = grids_for(ctx, n_new, n + 1);
  RFM_HIP_CHECK(hipMemsetAsync(hist, 0, size_t(n + 2) * 4, st));
  hipLaunchKernelGGL(fg_keys_counts_kernel, dim3(g2.elements), dim3(kFgBlock), 0, st, d_row_ptr, n_new, n, keys2, hist);
  group_counted(ctx, keys2, n_new, n + 1, hist, bin_ptr2, d_order, tiles, lists, w.list_cap);
}

}  // namespace
}  // namespace rfm

using namespace rfm;

extern "C" {

int32_t rfm_fold_group_workspace(int64_t n, int64_t n_new, int64_t* h_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_bytes, "null pointer");
    RFM_REQUIRE(n >= 0 && n < kLimit && n_new >= 0 && n_new < kLimit, "n=%lld, n_new=%lld out of range (0..2^31-1)",
                (long long)n, (long long)n_new);
    *h_bytes = Workspace(n, n_new).bytes;
  });
}

int32_t rfm_fold_group_geometry(const rfm_ctx* ctx, int64_t n, int64_t n_bins, int32_t* h_out8) {
  return guarded([&] {
    RFM_REQUIRE(h_out8, "null pointer");
    RFM_REQUIRE(n >= 0 && n < kLimit && n_bins >= 0 && n_bins <= kLimit, "n=%lld, n_bins=%lld out of range",
                (long long)n, (long long)n_bins);
    const rfm_ctx assumed{};  // (the CU count of an MI355X)
    const Grids g = grids_for(ctx ? ctx : &assumed, n, n_bins);
    h_out8[0] = kCap;
    h_out8[1] = kFgBlock;
    h_out8[2] = g.per_bin;
    h_out8[3] = kWaveCap;
    h_out8[4] = g.mid;
    h_out8[5] = g.lng;
    h_out8[6] = kLongBlock;
    h_out8[7] = g.elements;
  });
}

int32_t rfm_fold_group(rfm_ctx* ctx, const void* d_new, const void* d_other, int64_t id_stride, int32_t id_bytes,
                       const double* d_labels, const double* d_pscores, int64_t n, int64_t n_new, int64_t n_fixed,
                       void* d_workspace, int64_t workspace_bytes, int64_t* d_row_ptr, int32_t* d_ids, double* d_ry,
                       int32_t* d_order, int32_t* d_status) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_row_ptr && d_status, "null pointer");
    RFM_REQUIRE(n >= 0 && n < kLimit && n_new >= 0 && n_new < kLimit, "n=%lld, n_new=%lld out of range (0..2^31-1)",
                (long long)n, (long long)n_new);
    RFM_REQUIRE(n_fixed >= 0, "negative n_fixed");
    RFM_REQUIRE(id_bytes == 4 || id_bytes == 8, "ids of %d bytes (4 or 8)", id_bytes);
    RFM_REQUIRE(id_stride >= 1, "id_stride=%lld: at least 1", (long long)id_stride);
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RFM_HIP_CHECK(hipMemsetAsync(d_status, 0, 16, st));
    RFM_HIP_CHECK(hipMemsetAsync(d_status + 2, 0xff, 4, st));  // no bad example: -1
    RFM_HIP_CHECK(hipMemsetAsync(d_row_ptr, 0, size_t(n_new + 1) * 8, st));
    if (n_new == 0) return;
    RFM_REQUIRE(d_order, "null pointer");
    if (n == 0) {  // argsort of equal counts: every row in place
      hipLaunchKernelGGL(fg_iota_kernel, dim3(capped_grid(ctx, n_new, kFgBlock, kPerCu, 1)), dim3(kFgBlock), 0, st, d_order,
                         n_new);
      RFM_HIP_CHECK(hipGetLastError());
      return;
    }
    RFM_REQUIRE(d_new && d_other && d_labels && d_pscores && d_ids && d_ry && d_workspace, "null pointer");
    RFM_REQUIRE((uintptr_t(d_new) | uintptr_t(d_other)) % size_t(id_bytes) == 0, "id columns not aligned to %d bytes",
                id_bytes);
    RFM_REQUIRE(uintptr_t(d_workspace) % 16 == 0, "workspace not aligned to 16 bytes");
    RFM_REQUIRE(workspace_bytes >= Workspace(n, n_new).bytes, "workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)Workspace(n, n_new).bytes);
    if (id_bytes == 4)
      fold_group<int32_t>(ctx, d_new, d_other, id_stride, d_labels, d_pscores, n, n_new, n_fixed,
                          static_cast<char*>(d_workspace), d_row_ptr, d_ids, d_ry, d_order, d_status);
    else
      fold_group<int64_t>(ctx, d_new, d_other, id_stride, d_labels, d_pscores, n, n_new, n_fixed,
                          static_cast<char*>(d_workspace), d_row_ptr, d_ids, d_ry, d_order, d_status);
  });
}

}  // extern "C"
