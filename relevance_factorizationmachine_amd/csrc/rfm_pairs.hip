// Catalogue scoring and top-K: every (user, item) pair of a trained model
// without the design matrix of the pairs.
//
// A pair's FM row is the user's entries + the item's entries on disjoint columns,
// x(u,i) = xu(u) + xi(i).  With a_u = sum_j xu_j V[j,:], b_i = sum_j xi_j V[j,:] and, per side,
// L(x) = w.x + 0.5 sum_f((sum_j x_j V[j,f])^2 - sum_j x_j^2 V[j,f]^2), the reference's logit
// (src/fm.py:124-132) is exactly
//     logit(u,i) = w0 + L(xu) + L(xi) + a_u . b_i
// and MF's (src/mf.py:154-170) has the same shape with a = P, b = Q, L = b_u, b_i and the
// constant b.  Two kernels: the side sums (one wavefront per sparse row) and the pair tile, a
// dense [users x k].[k x items] product on the f64 matrix core (v_mfma_f64_16x16x4_f64) with
// two epilogues: sigmoid scores, or the K best items per user under the total order
// (logit descending, item index descending).  Every sum has a fixed order and no float
// atomic is used: the same inputs give the same bits.
//
// Ranks against the catalogue are two more epilogues of the same tile: one
// stores the logit of every target pair that falls into the tile, one counts, per target, the
// tile's candidates that are better than it.  The counts are integers, summed with integer
// atomics: they do not depend on the split or on timing.
//
// A user's ranking of the catalogue to any depth is a fifth epilogue, the raw
// logits of a block of users to a workspace, and a ranking kernel of its own: one workgroup per
// row, a streaming selection under the same total order with bitonic sorts and merges in LDS.
//
// Nearest neighbours in factor space are the top-K launches on one table against
// itself (or against a table of queries) with the value left as it is: a kernel that divides every
// row by its norm in a fixed order, and a merge instantiation whose last store skips the sigmoid.
//
// The item -> users direction is a second compile-time form of the tile: its rows
// are items, its columns users, and the epilogue still adds the user's side term first, so that a
// pair's logit has the same bytes in both directions.
#include <cmath>
#include <cstdlib>

#include "rfm_common.h"
#include "rfm_device_utils.hpp"

namespace rfm {
namespace {

constexpr int kPairBlock = 256;  // 4 wavefronts, 2 x 2 over the tile
constexpr int kTile = 64;        // users and items of a workgroup tile
constexpr int kChunk = 32;       // factors staged in LDS at a time
// LDS row stride (doubles) of one factor's 64 tile rows.  A k-step's ds_read_b64 takes lanes
// 0-31 (MFMA k-slots 0 and 1) in one LDS cycle; slot s reads factor s * 8 + step, so the two
// slots are 8 * 66 = 16 (mod 32) doubles apart and the 32 lanes fall on 32 distinct 8-byte
// bank pairs.  The staging writes (factor fastest) are 2-way conflicted: 1 write per 2+ reads.
constexpr int kLd = 66;
constexpr int kOperandDoubles = 2 * kChunk * kLd;  // A and B chunk
constexpr int kLogitLd = kTile + 1;                // top-K epilogue: the tile's logits [user][item]
// LDS doubles shared by the operand chunks and, after the product, the tile's logits
constexpr int kUnion = kOperandDoubles > kTile * kLogitLd ? kOperandDoubles : kTile * kLogitLd;
constexpr int64_t kMaxSel = int64_t(65535) * kTile;  // selected users of a launch: grid y
constexpr int kMaxTopK = 64;
constexpr int kTargetWorkgroups = 1024;  // top-K: item splits are chosen to reach about this many
// rank counting: a workgroup sums the counts of the first kRankAccum targets of its 64 users in
// LDS over its tiles (one atomic per target and workgroup); later targets go to memory per tile
constexpr int kRankAccum = 4096;

// epilogue of the pair tile
enum PairMode { kScores = 0, kTopK = 1, kTargetLogits = 2, kRankCount = 3, kLogits = 4 };
// what the tile's rows (the queries) and columns (the candidates) are
enum PairForm { kByUser = 0, kByItem = 1 };

using f64x4 = __attribute__((__vector_size__(4 * sizeof(double)))) double;

inline int64_t pad4(int64_t k) { return (k + 3) / 4 * 4; }

inline bool check_ids_enabled() {
  const char* v = std::getenv("RFM_CHECK_IDS");
  return v && std::atoi(v) != 0;
}

// ---------------------------------------------------------------------------
// side sums: A[r, 0:kpad] = sum_j S[r,j] V[j,:] (zero beyond k), L[r] as above.
// One wavefront per row, lanes over factors (64 at a time: coalesced V row reads), entries in
// stored order, the factors' partial sums reduced by a fixed xor tree.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPairBlock) void side_sums_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const double* __restrict__ values, int64_t n_rows, const double* __restrict__ w,
    const double* __restrict__ V, int64_t n_features, int k, int kpad, double* __restrict__ A,
    double* __restrict__ L, int32_t* flags) {
  const int lane = threadIdx.x & 63;
  const int64_t r = int64_t(blockIdx.x) * (kPairBlock / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int64_t lo = indptr[r], hi = indptr[r + 1];
  double lin = 0.0, cross = 0.0;
  for (int f0 = 0; f0 < kpad; f0 += 64) {
    const int f = f0 + lane;
    double s = 0.0, q = 0.0;
    for (int64_t e = lo; e < hi; ++e) {
      const int64_t col = indices[e];
      if (col < 0 || col >= n_features) {  // never read outside V; reported under RFM_CHECK_IDS
        if (flags && lane == 0) atomicOr(flags, 1);
        continue;
      }
      const double x = values[e];
      if (f0 == 0) lin += x * w[col];
      if (f < k) {
        const double v = V[col * int64_t(k) + f];
        s += x * v;
        q += (x * x) * (v * v);
      }
    }
    if (f < kpad) A[r * int64_t(kpad) + f] = s;
    cross += s * s - q;
  }
  for (int m = 32; m >= 1; m >>= 1) cross += __shfl_xor(cross, m, 64);
  if (lane == 0) L[r] = lin + 0.5 * cross;
}

// ---------------------------------------------------------------------------
// normalised rows: out[r, 0:k] = M[r, 0:k] / ||M[r, 0:k]||_2, zero beyond k,
// norms[r] = the norm.  One wavefront per row, the rows strided over a capped grid.  The order is
// fixed (include/rfm_neighbours.h states it): lane l adds the rounded squares of the factors l, l + 64,
// ... in ascending order, the 64 sums go through the side sums' xor tree, the root and every
// quotient are IEEE operations.  A norm that is zero, NaN or infinite gives NaN in 0 .. k-1.
// `wide`: M's rows and out start on 16 bytes, so the second pass moves two factors at a time.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPairBlock) void rows_normalise_kernel(
    const double* __restrict__ M, int64_t n_rows, int k, int kpad, int64_t ld, bool wide,
    double* __restrict__ out, double* __restrict__ norms) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t step = int64_t(gridDim.x) * (kPairBlock / 64);
  for (int64_t r = int64_t(blockIdx.x) * (kPairBlock / 64) + (threadIdx.x >> 6); r < n_rows; r += step) {
    const double* __restrict__ row = M + r * ld;
    double s = 0.0;
    for (int f = lane; f < k; f += 64) {
      // (the operators under the pragma above, as rfm_rule.hpp spells a rounded product and sum:
      // the bodies of __dmul_rn / __dadd_rn are inlined from a header it does not reach, and
      // their product and sum came out as one v_fmac_f64)
      const double x = row[f];
      const double xx = x * x;
      s = s + xx;
    }
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
    const double norm = __dsqrt_rn(s);
    const bool ok = norm > 0.0 && norm < INFINITY;  // (false for a NaN)
    if (lane == 0) norms[r] = norm;
    double* __restrict__ o = out + r * int64_t(kpad);
    if (wide) {
      for (int f = 2 * lane; f < kpad; f += 128) {  // (kpad is even: f + 1 < kpad)
        double2 x = make_double2(0.0, 0.0);
        if (f + 1 < k) x = *reinterpret_cast<const double2*>(row + f);
        else if (f < k) x.x = row[f];
        double2 y;
        y.x = f < k ? (ok ? __ddiv_rn(x.x, norm) : NAN) : 0.0;
        y.y = f + 1 < k ? (ok ? __ddiv_rn(x.y, norm) : NAN) : 0.0;
        *reinterpret_cast<double2*>(o + f) = y;
      }
    } else {
      for (int f = lane; f < kpad; f += 64) o[f] = f < k ? (ok ? __ddiv_rn(row[f], norm) : NAN) : 0.0;
    }
  }
}

// ---------------------------------------------------------------------------
// top-K lists.  Entry = (logit, item); an empty slot is (-inf, -1), which every real
// candidate beats.  Lane j of a wavefront holds entry j of a list sorted best first.
// ---------------------------------------------------------------------------
__device__ inline bool better(double la, int ia, double lb, int ib) {
  return la > lb || (la == lb && ia > ib);
}

// Value of lane `src` (wave-uniform) for every lane: v_readlane, no LDS round trip.
__device__ inline int lane_get(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ inline double lane_get(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src),
                          __builtin_amdgcn_readlane(__double2loint(v), src));
}
// Value of the lane below (lane 0 keeps its own): DPP wave_shr:1.
__device__ inline int lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false); }
__device__ inline double lane_below(double v) {
  return __hiloint2double(lane_below(__double2hiint(v)), lane_below(__double2loint(v)));
}

// Insert the candidates of the lanes named by `mask` (one per lane; wave-uniform) into the list
// held by lanes 0 .. K-1.  The order is total, so the result does not depend on the order of
// insertion.  Must be called with all 64 lanes active.
__device__ inline void list_insert(unsigned long long mask, double cl, int ci, int K, int lane,
                                   double& ml, int& mi) {
  while (mask) {
    const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
    mask &= mask - 1;
    const double l = lane_get(cl, b);
    const int i = lane_get(ci, b);
    if (!better(l, i, lane_get(ml, K - 1), lane_get(mi, K - 1))) continue;
    // the entries that stay in front of the candidate are a prefix of the list
    const int p = __popcll(__ballot(lane < K && better(ml, mi, l, i)));
    const double ul = lane_below(ml);
    const int ui = lane_below(mi);
    if (lane == p) {
      ml = l;
      mi = i;
    } else if (lane > p) {
      ml = ul;
      mi = ui;
    }
  }
}

// true if `item` is in the ascending list excl[lo, hi)
__device__ inline bool excluded(const int32_t* __restrict__ excl, int64_t lo, int64_t hi, int item) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int v = excl[mid];
    if (v == item) return true;
    if (v < item) lo = mid + 1; else hi = mid;
  }
  return false;
}

// Selected user s of a launch whose first is selected user `first` -> the user's id (user_of; for a
// user known to be in the table: its row) and -> row of the user table, or -1 for an id outside it,
// which `report` raises in `flags` if given (RFM_CHECK_IDS: bit 1).
__device__ inline int64_t user_of(const int32_t* user_ids, int64_t s, int64_t first) {
  return user_ids ? int64_t(user_ids[s]) : s + first;
}
__device__ inline int64_t user_row(const int32_t* user_ids, int64_t s, int64_t first, int64_t n_users,
                                   int32_t* flags = nullptr, bool report = false) {
  int64_t u = user_of(user_ids, s, first);
  if (u < 0 || u >= n_users) {
    if (flags && report) atomicOr(flags, 2);
    u = -1;
  }
  return u;
}

struct PairArgs {
  const double* A;         // [n_users][kpad]
  const double* LU;        // [n_users]
  const int32_t* user_ids; // [n_sel] or null (selected user s = user s)
  int64_t n_users, n_sel;
  const double* B;         // [n_items][kpad]
  const double* LI;        // [n_items]
  int64_t n_items;
  int kpad;
  const double* c;         // device scalar
  // scores epilogue
  double* out;             // [n_sel][n_items]
  // top-K epilogue
  const int64_t* excl_indptr;  // [n_users + 1] or null
  const int32_t* excl_items;
  int K, n_splits, tiles_per_split;
  double* ws_logit;        // [n_splits][n_sel][K]
  int32_t* ws_item;
  int32_t* flags;          // RFM_CHECK_IDS: bit 1 = a user id outside the table
  // rank epilogues: the targets of selected user s are tgt_items[tgt_indptr[s] .. tgt_indptr[s+1])
  const int64_t* tgt_indptr;   // [n_sel + 1]
  const int32_t* tgt_items;    // [n_targets], ascending per user
  int64_t n_targets;
  double* tgt_logit;           // [n_targets]: written by kTargetLogits, read by kRankCount
  int32_t* out_ranks;          // [n_targets], zeroed before kRankCount
  int32_t* out_candidates;     // [n_sel], zeroed before kRankCount
  // kLogits: the launch covers the selected users sel_first .. sel_first + n_sel - 1 (user_ids,
  // if given, already points at the first of them) and `out` takes their raw logits
  int64_t sel_first;
};

// logit[u,i] = c + LU[u] + LI[i] + A[u,:].B[i,:] over a 64 x 64 tile: wavefront (wm, wn) owns
// the 32 x 32 quarter at (32 wm, 32 wn) as 2 x 2 MFMA blocks of 16 x 16; the factors go
// through LDS in chunks of 32 so that each operand element is read from memory once per tile.
// kLogits is kScores without the sigmoid: one tile per workgroup, the raw logit
// stored to out[user of the launch][item], NaN for a user id outside the table.
// Every other mode: blockIdx.x is an item split; the workgroup walks the split's tiles and
// hands each tile's logits over in LDS (T[user][item]).  kTopK keeps the K best items of each of
// its 64 users in LDS lists, written to the workspace at the end.  kTargetLogits stores the logit
// of every target of its users that lies in the tile.  kRankCount turns excluded items into NaN
// and adds, per target of a user, the number of the tile's logits that are better than it.
// FORM kByItem: the host has exchanged the two tables (tile_sides), so "user"
// below reads "query item" and "item" reads "candidate user": A, LU, user_ids, n_users, the
// exclusion lists and the targets are by item, B, LI, n_items the users.  The one difference is the
// order of the two side terms in the epilogue, which stays user first.  The dot product needs no
// change: every product a * b commutes and the factors are taken in the same order, so the
// accumulator of (item i, user u) is that of (u, i) in the forward form (test_gpu_audience.py holds
// the two to the same bytes; the argument alone is not relied on).
template <int MODE, int FORM = kByUser>
__global__ __launch_bounds__(kPairBlock) void pair_tile_kernel(PairArgs a) {
  constexpr bool TOPK = MODE == kTopK;
  constexpr bool WALK = MODE != kScores && MODE != kLogits;  // item splits, logits through T
  extern __shared__ double lds[];
  double* As = lds;                    // [kChunk][kLd]
  double* Bs = lds + kChunk * kLd;     // [kChunk][kLd]
  double* T = lds;                     // TOPK epilogue, after the product: [kTile][kLogitLd]
  double* list_l = lds + kUnion;                                        // [kTile][K]
  int32_t* list_i = reinterpret_cast<int32_t*>(list_l + kTile * (TOPK ? a.K : 0));
  int32_t* rank_acc = reinterpret_cast<int32_t*>(lds + kUnion);  // kRankCount: [kRankAccum]
  int32_t* cand_acc = rank_acc + kRankAccum;                     // kRankCount: [kTile]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t u0 = int64_t(blockIdx.y) * kTile;
  const int kpad = a.kpad;
  const int64_t first = MODE == kLogits ? a.sel_first : 0;  // (compile time: the others take no add)

  // staging: thread -> factor tid & 31 of rows (tid >> 5) + 8 j: 256-byte runs of a row
  const int sk = tid & (kChunk - 1), sr = tid >> 5;
  const double* a_row[8];
  bool user_ok[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t s = u0 + sr + 8 * j;
    int64_t u = -1;
    if (s < a.n_sel) u = user_row(a.user_ids, s, first, a.n_users, a.flags, sk == 0);
    user_ok[j] = u >= 0;
    a_row[j] = a.A + (u >= 0 ? u : 0) * int64_t(kpad);
  }

  if (TOPK) {
    for (int e = tid; e < kTile * a.K; e += kPairBlock) {
      list_l[e] = -INFINITY;
      list_i[e] = -1;
    }
  }
  if (MODE == kRankCount) {
    for (int e = tid; e < kRankAccum + kTile; e += kPairBlock) rank_acc[e] = 0;
  }

  const int n_item_tiles = int((a.n_items + kTile - 1) / kTile);
  const int t_first = WALK ? blockIdx.x * a.tiles_per_split : blockIdx.x;
  const int t_last = WALK ? min(t_first + a.tiles_per_split, n_item_tiles) : t_first + 1;
  const double c = a.c[0];

  for (int t = t_first; t < t_last; ++t) {
    const int64_t i0 = int64_t(t) * kTile;
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};

    double ra[8], rb[8];  // the next chunk on its way from memory while this one is multiplied
    auto fetch = [&](int k0) {
      const int kk = k0 + sk;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t item = i0 + sr + 8 * j;
        ra[j] = (kk < kpad && user_ok[j]) ? a_row[j][kk] : 0.0;
        rb[j] = (kk < kpad && item < a.n_items) ? a.B[item * int64_t(kpad) + kk] : 0.0;
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < kpad; k0 += kChunk) {
      __syncthreads();  // the chunk before (or the epilogue's T, or the lists' init) is done with
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        As[sk * kLd + sr + 8 * j] = ra[j];
        Bs[sk * kLd + sr + 8 * j] = rb[j];
      }
      __syncthreads();
      if (k0 + kChunk < kpad) fetch(k0 + kChunk);
      // factors of this chunk (a multiple of 4): MFMA k-slot s takes the quarter [s q, s q + q)
      const int q = min(kChunk, kpad - k0) >> 2;
      const double* ap = As + ((lane >> 4) * q) * kLd + wm * 32 + (lane & 15);
      const double* bp = Bs + ((lane >> 4) * q) * kLd + wn * 32 + (lane & 15);
      for (int s = 0; s < q; ++s) {
        const double a0 = ap[s * kLd], a1 = ap[s * kLd + 16];
        const double b0 = bp[s * kLd], b1 = bp[s * kLd + 16];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }

    // C/D layout of the f64 MFMA: column (item) = lane & 15, row (user) = (lane >> 4) + 4 reg
    if (WALK) __syncthreads();  // every wavefront has read its operands: T may overwrite them
#pragma unroll
    for (int x = 0; x < 2; ++x) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ul = wm * 32 + x * 16 + (lane >> 4) + 4 * reg;
        const int64_t s = u0 + ul;
        int64_t u = -1;
        if (s < a.n_sel) u = user_row(a.user_ids, s, first, a.n_users);
        const double lu = u >= 0 ? a.LU[u] : NAN;  // a user id outside the table scores NaN
#pragma unroll
        for (int y = 0; y < 2; ++y) {
          const int il = wn * 32 + y * 16 + (lane & 15);
          const int64_t item = i0 + il;
          const bool in = s < a.n_sel && item < a.n_items;
          // ((c + LU[user]) + LI[item]) + acc in either form: by item the row's term is the item's
          const double logit = !in ? NAN
                               : FORM == kByItem ? ((c + a.LI[item]) + lu) + acc[x][y][reg]
                                                 : ((c + lu) + a.LI[item]) + acc[x][y][reg];
          if (WALK) {
            T[ul * kLogitLd + il] = logit;
          } else if (in) {
            a.out[s * a.n_items + item] = MODE == kLogits ? logit : sigmoid_clipped(logit);
          }
        }
      }
    }
    if (!WALK) continue;
    __syncthreads();
    if (MODE == kTargetLogits) {
      // wavefront w serves users 16 w .. 16 w + 15: the user's targets are ascending, the ones
      // of this tile start at the first id >= i0 (the same search in every lane) and the lanes
      // take them 64 at a time.  A target id outside the catalogue is in no tile: its logit
      // keeps the NaN the workspace was filled with.
      for (int j = 0; j < 16; ++j) {
        const int ul = wave * 16 + j;
        const int64_t s = u0 + ul;
        if (s >= a.n_sel) break;
        int64_t lo = max(a.tgt_indptr[s], int64_t(0));
        const int64_t thi = min(a.tgt_indptr[s + 1], a.n_targets);
        for (int64_t hi = thi; lo < hi;) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (int64_t(a.tgt_items[mid]) < i0) lo = mid + 1; else hi = mid;
        }
        for (int64_t p = lo + lane;; p += 64) {
          const int64_t it = p < thi ? int64_t(a.tgt_items[p]) : -1;
          const bool in = it >= i0 && it < i0 + kTile;
          if (in) a.tgt_logit[p] = T[ul * kLogitLd + int(it - i0)];
          if (__ballot(in) != ~0ull) break;
        }
      }
      continue;  // (the next tile's first barrier orders these reads of T before its staging writes)
    }
    if (MODE == kRankCount) {
      const int64_t tbase = max(a.tgt_indptr[u0], int64_t(0));  // (u0 < n_sel: the grid has no empty user tile)
      for (int j = 0; j < 16; ++j) {
        const int ul = wave * 16 + j;
        const int64_t s = u0 + ul;
        if (s >= a.n_sel) break;
        double* row = T + ul * kLogitLd;
        double cl = row[lane];
        if (a.excl_indptr) {
          if (cl == cl) {
            const int64_t u = user_of(a.user_ids, s, first);  // (in range: its logits are not NaN)
            if (excluded(a.excl_items, a.excl_indptr[u], a.excl_indptr[u + 1], int(i0) + lane)) cl = NAN;
          }
          row[lane] = cl;  // the wavefront's own row: its LDS accesses are executed in order
        }
        const int n_cand = __popcll(__ballot(cl == cl));
        if (n_cand == 0) continue;  // NaN beats nothing
        if (lane == 0) cand_acc[ul] += n_cand;
        // lane = one target of the user, 64 at a time; the tile's logits come as broadcast reads
        const int64_t tlo = max(a.tgt_indptr[s], int64_t(0)), thi = min(a.tgt_indptr[s + 1], a.n_targets);
        for (int64_t p0 = tlo; p0 < thi; p0 += 64) {
          const int64_t p = p0 + lane;
          const double tl = p < thi ? a.tgt_logit[p] : NAN;  // NaN is beaten by nothing
          const int ti = p < thi ? a.tgt_items[p] : 0;
          int cnt = 0;
#pragma unroll 8
          for (int e = 0; e < kTile; ++e) {  // better(row[e], i0 + e, tl, ti) without its branches
            const double l = row[e];
            cnt += int(l > tl) + int((l == tl) & (int(i0) + e > ti));
          }
          if (cnt) {
            const int64_t at = p - tbase;
            if (at >= 0 && at < kRankAccum) rank_acc[at] += cnt;  // target p belongs to this lane alone
            else atomicAdd(a.out_ranks + p, cnt);
          }
        }
      }
      continue;
    }
    // wavefront w ranks users 16 w .. 16 w + 15, lane = item of the tile.  A candidate is
    // looked at further only if it beats the list's current K-th entry; after the first tiles
    // almost none does.  NaN logits (and the tile's padding) are never ranked.
    for (int j = 0; j < 16; ++j) {
      const int ul = wave * 16 + j;
      const int64_t s = u0 + ul;
      if (s >= a.n_sel) break;
      const double cl = T[ul * kLogitLd + lane];
      const int ci = int(i0) + lane;
      double* ll = list_l + ul * a.K;
      int32_t* li = list_i + ul * a.K;
      bool pass = cl == cl && better(cl, ci, ll[a.K - 1], li[a.K - 1]);
      if (__ballot(pass) == 0) continue;
      if (pass && a.excl_indptr) {
        const int64_t u = user_of(a.user_ids, s, first);  // (in range: its logits are not NaN)
        pass = !excluded(a.excl_items, a.excl_indptr[u], a.excl_indptr[u + 1], ci);
      }
      unsigned long long mask = __ballot(pass);
      if (mask == 0) continue;
      if (__popcll(mask) > a.K) {
        // (a split's first tiles) only the K best of the tile's own candidates can enter the
        // list: every lane counts the candidates that beat its own, in parallel, which is much
        // cheaper than letting the serial insertion below turn the others away one by one
        int rank = 0;
        for (unsigned long long m = mask; m; m &= m - 1) {
          const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
          rank += better(lane_get(cl, b), lane_get(ci, b), cl, ci) ? 1 : 0;
        }
        pass = pass && rank < a.K;
        mask = __ballot(pass);
      }
      double ml = lane < a.K ? ll[lane] : -INFINITY;
      int mi = lane < a.K ? li[lane] : -1;
      list_insert(mask, cl, ci, a.K, lane, ml, mi);
      if (lane < a.K) {
        ll[lane] = ml;
        li[lane] = mi;
      }
    }
    // (the next tile's first barrier orders these reads of T before its staging writes)
  }

  if (MODE == kRankCount) {
    __syncthreads();
    const int64_t tbase = max(a.tgt_indptr[u0], int64_t(0));
    for (int e = tid; e < kRankAccum; e += kPairBlock)
      if (rank_acc[e] && tbase + e < a.n_targets) atomicAdd(a.out_ranks + tbase + e, rank_acc[e]);
    if (tid < kTile && u0 + tid < a.n_sel && cand_acc[tid]) atomicAdd(a.out_candidates + u0 + tid, cand_acc[tid]);
  }
  if (TOPK) {
    // a wavefront wrote the lists it now copies out: no barrier needed
    for (int j = 0; j < 16; ++j) {
      const int ul = wave * 16 + j;
      const int64_t s = u0 + ul;
      if (s >= a.n_sel) break;
      if (lane < a.K) {
        const int64_t at = (int64_t(blockIdx.x) * a.n_sel + s) * a.K + lane;
        a.ws_logit[at] = list_l[ul * a.K + lane];
        a.ws_item[at] = list_i[ul * a.K + lane];
      }
    }
  }
}

// One wavefront per selected user: the splits' partial lists (each sorted) into the final one;
// scores = sigmoid(logit), RAW: the logit itself (rfm_pair_topk_raw); an empty slot = item -1 /
// score NaN.
template <bool RAW>
__global__ __launch_bounds__(kPairBlock) void topk_merge_kernel(
    const double* __restrict__ ws_logit, const int32_t* __restrict__ ws_item, int n_splits,
    int64_t n_sel, int K, int32_t* __restrict__ out_items, double* __restrict__ out_scores) {
  const int lane = threadIdx.x & 63;
  const int64_t s = int64_t(blockIdx.x) * (kPairBlock / 64) + (threadIdx.x >> 6);
  if (s >= n_sel) return;
  double ml = -INFINITY;
  int mi = -1;
  for (int p = 0; p < n_splits; ++p) {
    const int64_t at = (int64_t(p) * n_sel + s) * K + lane;
    const double cl = lane < K ? ws_logit[at] : -INFINITY;
    const int ci = lane < K ? ws_item[at] : -1;
    const double tl = lane_get(ml, K - 1);
    const int ti = lane_get(mi, K - 1);
    const bool pass = ci >= 0 && better(cl, ci, tl, ti);
    const unsigned long long mask = __ballot(pass);
    if (mask) list_insert(mask, cl, ci, K, lane, ml, mi);
  }
  if (lane < K) {
    out_items[s * K + lane] = mi;
    out_scores[s * K + lane] = mi >= 0 ? (RAW ? ml : sigmoid_clipped(ml)) : NAN;
  }
}

// RFM_CHECK_IDS=1: indptr monotone from 0, every list strictly ascending inside 0 .. n_items-1
__global__ __launch_bounds__(kPairBlock) void excl_check_kernel(const int64_t* indptr,
                                                               const int32_t* items, int64_t n_users,
                                                               int64_t n_items, int32_t* flags) {
  for (int64_t u = int64_t(blockIdx.x) * kPairBlock + threadIdx.x; u < n_users;
       u += int64_t(gridDim.x) * kPairBlock) {
    const int64_t lo = indptr[u], hi = indptr[u + 1];
    if ((u == 0 && lo != 0) || hi < lo) {
      atomicOr(flags, 4);
      continue;
    }
    for (int64_t e = lo; e < hi; ++e)
      if (items[e] < 0 || items[e] >= n_items || (e > lo && items[e] <= items[e - 1])) {
        atomicOr(flags, 8);
        break;
      }
  }
}

// RFM_CHECK_IDS=1: target indptr monotone from 0 up to n_targets, every list ascending (repeats
// allowed) inside 0 .. n_items-1; null items = the indptr only
__global__ __launch_bounds__(kPairBlock) void target_check_kernel(const int64_t* indptr,
                                                                 const int32_t* items, int64_t n_sel,
                                                                 int64_t n_items, int64_t n_targets,
                                                                 int32_t* flags) {
  for (int64_t s = int64_t(blockIdx.x) * kPairBlock + threadIdx.x; s < n_sel;
       s += int64_t(gridDim.x) * kPairBlock) {
    const int64_t lo = indptr[s], hi = indptr[s + 1];
    if ((s == 0 && lo != 0) || hi < lo || hi > n_targets || (s == n_sel - 1 && hi != n_targets)) {
      atomicOr(flags, 16);
      continue;
    }
    for (int64_t e = lo; items && e < hi; ++e)
      if (items[e] < 0 || items[e] >= n_items || (e > lo && items[e] < items[e - 1])) {
        atomicOr(flags, 32);
        break;
      }
  }
}

// Per target: a NaN logit (NaN item row, user or item id outside its table) has rank -1 and
// score NaN; every other target keeps its count and gets sigmoid(logit).
__global__ __launch_bounds__(kPairBlock) void rank_finish_kernel(const double* __restrict__ tgt_logit,
                                                                int64_t n_targets,
                                                                int32_t* __restrict__ out_ranks,
                                                                double* __restrict__ out_scores) {
  for (int64_t t = int64_t(blockIdx.x) * kPairBlock + threadIdx.x; t < n_targets;
       t += int64_t(gridDim.x) * kPairBlock) {
    const double z = tgt_logit[t];
    if (z != z) out_ranks[t] = -1;
    out_scores[t] = z == z ? sigmoid_clipped(z) : NAN;
  }
}

// ---------------------------------------------------------------------------
// A user's ranking of the catalogue to any depth: one workgroup per row of raw
// logits (kLogits), a streaming selection under better().  LDS holds the P best entries seen so
// far, sorted best first, and a staging area of P; logits and items in separate arrays (8- and
// 4-byte strides: the compare-exchanges of a wavefront fall on distinct banks).  The threads walk
// the row kOrderPass(P) items at a time and append, through an integer LDS counter, the
// candidates that beat the current P-th entry; a staging area that could not take another pass
// is sorted (bitonic) and merged (half-cleaner + bitonic merge) into the best.  The order is
// total, so neither the order of appending nor the places of the flushes change the result.
// Depths above kOrderMaxP go in pages: a page ranks only what comes strictly after the row's
// cutoff, the last entry of the page before.
// ---------------------------------------------------------------------------
constexpr int kOrderMaxP = 4096;        // entries of the list = ranks of a page
constexpr int kOrderMinP = kPairBlock;  // (a pass appends up to one item per thread)

inline int order_list_len(int64_t n_ranks) {  // power of two >= min(n_ranks, kOrderMaxP)
  int p = kOrderMinP;
  while (p < kOrderMaxP && p < n_ranks) p <<= 1;
  return p;
}
__host__ __device__ inline int order_pass(int P) { return P < 4 * kPairBlock ? P : 4 * kPairBlock; }

struct OrderArgs {
  const double* logits;        // [rows of the launch][n_items]
  int64_t n_items;
  const int32_t* user_ids;     // of the launch's first row, or null (row r = user sel_first + r)
  int64_t sel_first, n_users;
  const int64_t* excl_indptr;  // [n_users + 1] or null
  const int32_t* excl_items;
  int P;                       // list length: a power of two, kOrderMinP .. kOrderMaxP
  int first_page;              // no cutoff; counts the candidates
  int64_t depth;               // columns of the outputs
  int64_t col0, n_cols;        // the page ranks columns col0 .. col0 + n_cols - 1, n_cols <= P
  int64_t fill_to;             // columns up to fill_to - 1 get the padding (the last page: depth)
  double* cut_l;               // [rows]: the page's last entry, the cutoff of the next page
  int32_t* cut_i;              //         (item -1: the row has no further candidate)
  int32_t* out_items;          // [rows][depth]
  double* out_scores;
  int32_t* out_n_ranked;       // [rows]
};

// entries i < j of a list: the better one goes to i (better_first) or to j
__device__ inline void order_cmpx(double* l, int32_t* it, int i, int j, bool better_first) {
  const double li = l[i], lj = l[j];
  const int ii = it[i], ij = it[j];
  if (better_first ? better(lj, ij, li, ii) : better(li, ii, lj, ij)) {
    l[i] = lj, l[j] = li;
    it[i] = ij, it[j] = ii;
  }
}

// The n staged entries into the best P.  Called by the whole workgroup after a barrier that
// follows the last append; ends with a barrier, the counter back at 0.
__device__ inline void order_flush(double* bl, int32_t* bi, double* sl, int32_t* si, int P, int n, int* count) {
  const int tid = threadIdx.x;
  int m = 1;
  while (m < n) m <<= 1;
  for (int e = n + tid; e < m; e += kPairBlock) {  // empty slots: beaten by every candidate
    sl[e] = -INFINITY;
    si[e] = -1;
  }
  __syncthreads();
  if (tid == 0) *count = 0;
  for (int k = 2; k <= m; k <<= 1) {  // bitonic sort of the m staged entries, best first
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < (m >> 1); t += kPairBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        order_cmpx(sl, si, i, i | j, (i & k) == 0);
      }
      __syncthreads();
    }
  }
  // best[P - 1 - t] against staged[t]: the P best of both, as a bitonic sequence
  for (int t = tid; t < m; t += kPairBlock) {
    const int b = P - 1 - t;
    if (better(sl[t], si[t], bl[b], bi[b])) {
      bl[b] = sl[t];
      bi[b] = si[t];
    }
  }
  __syncthreads();
  for (int j = P >> 1; j >= 1; j >>= 1) {
    for (int t = tid; t < (P >> 1); t += kPairBlock) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      order_cmpx(bl, bi, i, i | j, true);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPairBlock) void order_rows_kernel(OrderArgs a) {
  extern __shared__ double lds[];
  __shared__ int s_count, s_cand;
  const int P = a.P, pass = order_pass(P);
  double* bl = lds;       // [P] the best, sorted best first
  double* sl = lds + P;   // [P] staging
  int32_t* bi = reinterpret_cast<int32_t*>(lds + 2 * P);
  int32_t* si = bi + P;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const double* z = a.logits + row * a.n_items;
  int32_t* oi = a.out_items + row * a.depth;
  double* os = a.out_scores + row * a.depth;

  double cl = 0.0;
  int ci = 0;
  if (!a.first_page) {
    cl = a.cut_l[row];
    ci = a.cut_i[row];
    if (ci < 0) {  // (the whole workgroup) the row ended on an earlier page
      for (int64_t col = a.col0 + tid; col < a.fill_to; col += kPairBlock) {
        oi[col] = -1;
        os[col] = NAN;
      }
      return;
    }
  }
  int64_t elo = 0, ehi = 0;
  if (a.excl_indptr) {
    const int64_t u = user_row(a.user_ids, row, a.sel_first, a.n_users);
    if (u >= 0) elo = a.excl_indptr[u], ehi = a.excl_indptr[u + 1];  // (else every logit is NaN)
  }
  for (int e = tid; e < P; e += kPairBlock) {
    bl[e] = -INFINITY;
    bi[e] = -1;
  }
  if (tid == 0) s_count = 0, s_cand = 0;
  __syncthreads();

  int n_cand = 0;
  for (int64_t i0 = 0; i0 < a.n_items; i0 += pass) {
    const int staged = s_count;
    __syncthreads();  // everybody has read the counter before anybody appends
    if (staged > P - pass) order_flush(bl, bi, sl, si, P, staged, &s_count);
    const double tl = bl[P - 1];
    const int ti = bi[P - 1];
    for (int64_t i = i0 + tid; i < min(i0 + pass, a.n_items); i += kPairBlock) {
      const double l = z[i];
      bool ok = l == l;
      if (a.first_page) {
        if (ok && elo < ehi) ok = !excluded(a.excl_items, elo, ehi, int(i));
        n_cand += ok ? 1 : 0;
        ok = ok && better(l, int(i), tl, ti);
      } else {
        ok = ok && better(cl, ci, l, int(i)) && better(l, int(i), tl, ti);
        if (ok && elo < ehi) ok = !excluded(a.excl_items, elo, ehi, int(i));
      }
      if (ok) {
        const int at = atomicAdd(&s_count, 1);  // < P: at most `pass` appends since staged <= P - pass
        sl[at] = l;
        si[at] = int(i);
      }
    }
    __syncthreads();
  }
  const int staged = s_count;
  if (a.first_page && n_cand) atomicAdd(&s_cand, n_cand);
  __syncthreads();
  if (staged > 0) order_flush(bl, bi, sl, si, P, staged, &s_count);

  for (int64_t e = tid; a.col0 + e < a.fill_to; e += kPairBlock) {
    const int it = e < a.n_cols ? bi[e] : -1;
    oi[a.col0 + e] = it;
    os[a.col0 + e] = it >= 0 ? sigmoid_clipped(bl[e]) : NAN;
  }
  if (tid == 0) {
    a.cut_l[row] = bl[a.n_cols - 1];
    a.cut_i[row] = bi[a.n_cols - 1];
    if (a.first_page) a.out_n_ranked[row] = s_cand;
  }
}

// rfm_pair_order's workspace: per user of a block a row of logits and a cutoff
inline int64_t order_row_bytes(int64_t n_items) { return n_items * 8 + 12; }

struct Split {
  int n_splits, tiles_per_split;
};

// item splits of the top-K launch: a function of the sizes only (the workspace is sized by it)
Split topk_split(int64_t n_sel, int64_t n_items) {
  const int64_t user_tiles = std::max<int64_t>(1, (n_sel + kTile - 1) / kTile);
  const int64_t item_tiles = std::max<int64_t>(1, (n_items + kTile - 1) / kTile);
  const int64_t want = std::max<int64_t>(1, std::min(item_tiles, (kTargetWorkgroups + user_tiles - 1) / user_tiles));
  Split s;
  s.tiles_per_split = int((item_tiles + want - 1) / want);
  s.n_splits = int((item_tiles + s.tiles_per_split - 1) / s.tiles_per_split);
  return s;
}

size_t rank_lds_bytes(bool count) {
  return size_t(kUnion) * 8 + (count ? size_t(kRankAccum + kTile) * 4 : 0);
}

size_t topk_lds_bytes(int K) {
  return size_t(kUnion) * 8 + size_t(kTile) * K * 12;
}

// The checks and the fields that every rfm_pair_* entry shares; the entry adds its own fields.
PairArgs pair_args(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                   const int32_t* d_user_ids, int64_t n_sel, const double* d_B, const double* d_LI,
                   int64_t n_items, int32_t n_factors, const double* d_c, const int64_t* d_excl_indptr,
                   const int32_t* d_excl_items) {
  RFM_REQUIRE(ctx && d_A && d_LU && d_B && d_LI && d_c, "null pointer");
  RFM_REQUIRE(n_factors >= 1 && n_factors <= RFM_MAX_FACTORS, "n_factors=%d unsupported (1..%d)",
              n_factors, RFM_MAX_FACTORS);
  RFM_REQUIRE(n_users >= 1 && n_items >= 1, "empty user or item table");
  RFM_REQUIRE(n_sel >= 0 && n_sel <= kMaxSel, "n_sel_users=%lld outside 0..%lld", (long long)n_sel,
              (long long)kMaxSel);
  RFM_REQUIRE(n_items < (int64_t(1) << 31) - kTile, "n_items=%lld does not fit int32 item ids",
              (long long)n_items);
  RFM_REQUIRE(d_user_ids || n_sel == n_users, "without user ids every user is selected");
  RFM_REQUIRE(!d_excl_indptr || d_excl_items, "exclusion lists without items");
  PairArgs a{};
  a.A = d_A, a.LU = d_LU, a.user_ids = d_user_ids, a.n_users = n_users, a.n_sel = n_sel;
  a.B = d_B, a.LI = d_LI, a.n_items = n_items, a.kpad = int(pad4(n_factors)), a.c = d_c;
  a.excl_indptr = d_excl_indptr, a.excl_items = d_excl_items;
  return a;
}

// The one place where the by-item entries differ from their twins on the host: the item table
// becomes the tile's rows and the user table its columns.  Everything after it -- the checks of
// pair_args, the splits, the workspaces, the launches -- is the twin's code for the exchanged counts.
template <int FORM>
inline void tile_sides(const double*& d_A, const double*& d_LU, int64_t& n_users, const double*& d_B,
                       const double*& d_LI, int64_t& n_items) {
  if (FORM == kByItem) {
    std::swap(d_A, d_B);
    std::swap(d_LU, d_LI);
    std::swap(n_users, n_items);
  }
}

// flags of a checked call (RFM_CHECK_IDS=1): read back after a synchronisation
struct IdCheck {
  DevBuf buf;
  rfm_ctx* ctx;
  explicit IdCheck(rfm_ctx* c) : ctx(c) {
    if (!check_ids_enabled()) return;
    buf.alloc(4);
    RFM_HIP_CHECK(hipMemsetAsync(buf.p, 0, 4, ctx->stream));
  }
  int32_t* flags() const { return buf.as<int32_t>(); }
  // Reports what the launches so far have flagged and arms the flags again.
  void finish() {
    if (!buf.p) return;
    int32_t h = 0;
    RFM_HIP_CHECK(hipMemcpyAsync(&h, buf.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    RFM_HIP_CHECK(hipMemsetAsync(buf.p, 0, 4, ctx->stream));
    RFM_REQUIRE(!(h & 1), "a column index lies outside 0..n_features-1");
    RFM_REQUIRE(!(h & 2), "a user id lies outside 0..n_users-1");
    RFM_REQUIRE(!(h & 4), "the exclusion indptr is not monotone from 0");
    RFM_REQUIRE(!(h & 8), "an exclusion list is not strictly ascending inside 0..n_items-1");
    RFM_REQUIRE(!(h & 16), "the target indptr is not monotone from 0 to n_targets");
    RFM_REQUIRE(!(h & 32), "a target list is not ascending inside 0..n_items-1");
  }
  // The flags pointer of a pair launch and, before any of its lists is searched, their check.
  void begin(PairArgs& a) {
    a.flags = flags();
    if (!a.flags || !a.excl_indptr) return;
    hipLaunchKernelGGL(excl_check_kernel, dim3(capped_grid(ctx, a.n_users, kPairBlock, 16, 1)), dim3(kPairBlock),
                       0, ctx->stream, a.excl_indptr, a.excl_items, a.n_users, a.n_items, a.flags);
    RFM_HIP_CHECK(hipGetLastError());
    finish();
  }
  void check_targets(const int64_t* d_indptr, const int32_t* d_items, int64_t n_sel, int64_t n_items,
                     int64_t n_targets) {
    if (!flags()) return;
    hipLaunchKernelGGL(target_check_kernel, dim3(capped_grid(ctx, n_sel, kPairBlock, 16, 1)), dim3(kPairBlock), 0,
                       ctx->stream, d_indptr, d_items, n_sel, n_items, n_targets, flags());
    RFM_HIP_CHECK(hipGetLastError());
    finish();
  }
};

template <int FORM>
LdsLimits g_topk_lds;  // (per kernel function)
LdsLimits g_order_lds;

// rfm_pair_topk / rfm_pair_topk_raw: the same launches; RAW is the merge's last store alone
template <bool RAW, int FORM = kByUser>
void pair_topk_run(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users, const int32_t* d_user_ids,
                   int64_t n_sel_users, const double* d_B, const double* d_LI, int64_t n_items, int32_t n_factors,
                   const double* d_c, const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t k,
                   void* d_workspace, int32_t* d_out_items, double* d_out_scores) {
  RFM_REQUIRE(k >= 1 && k <= kMaxTopK, "k=%d outside 1..%d", k, kMaxTopK);
  tile_sides<FORM>(d_A, d_LU, n_users, d_B, d_LI, n_items);
  PairArgs a = pair_args(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                         d_excl_indptr, d_excl_items);
  if (n_sel_users == 0) return;
  RFM_REQUIRE(d_workspace && d_out_items && d_out_scores, "null workspace or output");
  RFM_HIP_CHECK(hipSetDevice(ctx->device));
  IdCheck chk(ctx);
  chk.begin(a);
  const Split sp = topk_split(n_sel_users, n_items);
  a.K = k, a.n_splits = sp.n_splits, a.tiles_per_split = sp.tiles_per_split;
  a.ws_logit = static_cast<double*>(d_workspace);
  a.ws_item = reinterpret_cast<int32_t*>(a.ws_logit + int64_t(sp.n_splits) * n_sel_users * k);
  const size_t lds = topk_lds_bytes(k);
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(&pair_tile_kernel<kTopK, FORM>), lds, g_topk_lds<FORM>);
  const dim3 grid((unsigned)sp.n_splits, (unsigned)((n_sel_users + kTile - 1) / kTile));
  hipLaunchKernelGGL((pair_tile_kernel<kTopK, FORM>), grid, dim3(kPairBlock), lds, ctx->stream, a);
  RFM_HIP_CHECK(hipGetLastError());
  const int64_t mgrid = (n_sel_users + kPairBlock / 64 - 1) / (kPairBlock / 64);
  hipLaunchKernelGGL(topk_merge_kernel<RAW>, dim3((unsigned)mgrid), dim3(kPairBlock), 0, ctx->stream,
                     a.ws_logit, a.ws_item, sp.n_splits, n_sel_users, int(k), d_out_items, d_out_scores);
  RFM_HIP_CHECK(hipGetLastError());
  chk.finish();
}

// rfm_pair_ranks / rfm_pair_ranks_n: `h_n_targets` null = the number of targets is read back from
// the end of the device indptr (which synchronises); everything after that is the same code
template <int FORM = kByUser>
void pair_ranks_run(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                    const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B, const double* d_LI,
                    int64_t n_items, int32_t n_factors, const double* d_c, const int64_t* d_excl_indptr,
                    const int32_t* d_excl_items, const int64_t* d_tgt_indptr, const int32_t* d_tgt_items,
                    const int64_t* h_n_targets, void* d_workspace, int32_t* d_out_ranks, double* d_out_scores,
                    int32_t* d_out_candidates) {
  tile_sides<FORM>(d_A, d_LU, n_users, d_B, d_LI, n_items);
  PairArgs a = pair_args(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                         d_excl_indptr, d_excl_items);
  if (n_sel_users == 0) return;
  RFM_REQUIRE(d_tgt_indptr && d_out_candidates, "null target indptr or candidates output");
  RFM_HIP_CHECK(hipSetDevice(ctx->device));
  int64_t n_targets = 0;
  if (h_n_targets) {
    n_targets = *h_n_targets;
    RFM_REQUIRE(n_targets >= 0 && n_targets < (int64_t(1) << 40), "n_targets=%lld", (long long)n_targets);
  } else {
    // the number of targets is the last entry of the indptr: the launches are sized by it
    RFM_HIP_CHECK(hipMemcpyAsync(&n_targets, d_tgt_indptr + n_sel_users, 8, hipMemcpyDeviceToHost, ctx->stream));
    RFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    RFM_REQUIRE(n_targets >= 0 && n_targets < (int64_t(1) << 40), "d_tgt_indptr ends at %lld targets", (long long)n_targets);
  }
  RFM_REQUIRE(n_targets == 0 || (d_tgt_items && d_workspace && d_out_ranks && d_out_scores),
              "null target items, workspace or output");
  IdCheck chk(ctx);
  chk.begin(a);
  chk.check_targets(d_tgt_indptr, d_tgt_items, n_sel_users, n_items, n_targets);
  const Split sp = topk_split(n_sel_users, n_items);
  a.n_splits = sp.n_splits, a.tiles_per_split = sp.tiles_per_split;
  a.tgt_indptr = d_tgt_indptr, a.tgt_items = d_tgt_items, a.n_targets = n_targets;
  a.tgt_logit = static_cast<double*>(d_workspace);
  a.out_ranks = d_out_ranks, a.out_candidates = d_out_candidates;
  const dim3 grid((unsigned)sp.n_splits, (unsigned)((n_sel_users + kTile - 1) / kTile));
  RFM_HIP_CHECK(hipMemsetAsync(d_out_candidates, 0, size_t(n_sel_users) * 4, ctx->stream));
  if (n_targets > 0) {
    // every byte 0xFF is a NaN: the logit of a target that no tile holds
    RFM_HIP_CHECK(hipMemsetAsync(d_workspace, 0xFF, size_t(n_targets) * 8, ctx->stream));
    RFM_HIP_CHECK(hipMemsetAsync(d_out_ranks, 0, size_t(n_targets) * 4, ctx->stream));
    const size_t lds1 = rank_lds_bytes(false);  // (both passes stay under the 64 KiB a launch may ask for as it is)
    hipLaunchKernelGGL((pair_tile_kernel<kTargetLogits, FORM>), grid, dim3(kPairBlock), lds1, ctx->stream, a);
    RFM_HIP_CHECK(hipGetLastError());
  }
  const size_t lds2 = rank_lds_bytes(true);
  hipLaunchKernelGGL((pair_tile_kernel<kRankCount, FORM>), grid, dim3(kPairBlock), lds2, ctx->stream, a);
  RFM_HIP_CHECK(hipGetLastError());
  if (n_targets > 0) {
    hipLaunchKernelGGL(rank_finish_kernel, dim3(capped_grid(ctx, n_targets, kPairBlock, 16, 1)),
                       dim3(kPairBlock), 0, ctx->stream, a.tgt_logit, n_targets, d_out_ranks, d_out_scores);
    RFM_HIP_CHECK(hipGetLastError());
  }
  chk.finish();
}

// rfm_pair_order / rfm_pair_order_by_item: blocks of users (by item: of items), per block the raw
// logits of the block and the ranking kernel's pages over them
template <int FORM = kByUser>
void pair_order_run(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                    const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                    const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                    const int64_t* d_excl_indptr, const int32_t* d_excl_items, int64_t depth,
                    void* d_workspace, int64_t workspace_bytes, int32_t* d_out_items,
                    double* d_out_scores, int32_t* d_out_n_ranked) {
  RFM_REQUIRE(depth >= 1, "depth=%lld: the ranking depth must be at least 1", (long long)depth);
  tile_sides<FORM>(d_A, d_LU, n_users, d_B, d_LI, n_items);
  PairArgs all = pair_args(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                           d_excl_indptr, d_excl_items);
  if (n_sel_users == 0) return;
  RFM_REQUIRE(d_workspace && d_out_items && d_out_scores && d_out_n_ranked, "null workspace or output");
  const int64_t block_rows = workspace_bytes / order_row_bytes(n_items) / kTile * kTile;
  RFM_REQUIRE(block_rows >= kTile, "workspace_bytes=%lld is less than one block of %d users (%lld bytes)",
              (long long)workspace_bytes, kTile, (long long)(kTile * order_row_bytes(n_items)));
  RFM_HIP_CHECK(hipSetDevice(ctx->device));
  IdCheck chk(ctx);
  chk.begin(all);
  // ranks beyond the catalogue are padding whatever the logits: they take no page of their own
  const int64_t n_ranks = std::min(depth, n_items);
  const int P = order_list_len(n_ranks);
  const size_t lds = size_t(P) * 2 * 12;
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(&order_rows_kernel), lds, g_order_lds);
  double* ws_logits = static_cast<double*>(d_workspace);
  double* ws_cut_l = ws_logits + block_rows * n_items;
  int32_t* ws_cut_i = reinterpret_cast<int32_t*>(ws_cut_l + block_rows);
  for (int64_t first = 0; first < n_sel_users; first += block_rows) {
    const int64_t rows = std::min(block_rows, n_sel_users - first);
    PairArgs a = all;  // this block of the selected users
    a.user_ids = d_user_ids ? d_user_ids + first : nullptr, a.n_sel = rows, a.sel_first = first;
    a.out = ws_logits;
    const dim3 grid((unsigned)((n_items + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile));
    hipLaunchKernelGGL((pair_tile_kernel<kLogits, FORM>), grid, dim3(kPairBlock), size_t(kOperandDoubles) * 8,
                       ctx->stream, a);
    RFM_HIP_CHECK(hipGetLastError());
    OrderArgs o{};
    o.logits = ws_logits, o.n_items = n_items, o.user_ids = a.user_ids, o.sel_first = first, o.n_users = n_users;
    o.excl_indptr = d_excl_indptr, o.excl_items = d_excl_items, o.P = P, o.depth = depth;
    o.cut_l = ws_cut_l, o.cut_i = ws_cut_i;
    o.out_items = d_out_items + first * depth, o.out_scores = d_out_scores + first * depth;
    o.out_n_ranked = d_out_n_ranked + first;
    for (int64_t col0 = 0; col0 < n_ranks; col0 += P) {  // (more than one page only with P = kOrderMaxP)
      o.first_page = col0 == 0, o.col0 = col0, o.n_cols = std::min<int64_t>(P, n_ranks - col0);
      o.fill_to = col0 + o.n_cols < n_ranks ? col0 + o.n_cols : depth;
      hipLaunchKernelGGL(order_rows_kernel, dim3((unsigned)rows), dim3(kPairBlock), lds, ctx->stream, o);
      RFM_HIP_CHECK(hipGetLastError());
    }
  }
  chk.finish();
}

// ---------------------------------------------------------------------------
// Catalogue metrics from ranks: DCG@K, Recall@K, MAP@K, MRR and AUC of the
// reference's calc_dcg_at_k / calc_recall_at_k / calc_average_precision_at_k
// (utils/metrics.py:9-107) as they come out for the 0/1 vector of a user's candidates, from the
// ranks of the user's positives alone (evaluate.CatalogueEvaluator.metrics states the sums).
// One wavefront per selected user, two steps.  Step 1 puts the user's ranked positives in
// ascending rank order by counting: the place of a positive is the number of the user's ranked
// positives below it (equal ranks, which distinct targets never have, go by position), 64
// positives against 64 at a time through v_readlane.  Step 2 walks the ordered ranks 64 at a
// time; lane c owns output column c (DCG@K_c, Recall@K_c, MAP@K_c) and adds the terms one by one
// in ascending rank order.  The sum of the ranks (AUC) is an integer.  A second launch takes the
// mean of every column over the users in a fixed order: no float atomic anywhere.
// ---------------------------------------------------------------------------
constexpr int kMaxMetricK = 16;

struct MetricArgs {
  const int64_t* tgt_indptr;   // [n_sel + 1]
  const int32_t* ranks;        // [n_targets], -1 = unranked
  const int32_t* candidates;   // [n_sel]
  const double* weights;       // [n_targets] or null (all ones): DCG only
  int64_t n_sel, n_targets;
  int n_K;
  int64_t K[kMaxMetricK], max_K;
  double* user_vals;           // [n_sel][3 n_K + 2]: DCG | Recall | MAP | MRR | AUC, NaN = not counted
  int32_t* sorted_rank;        // [n_targets]: per user, the ranked positives' ranks ascending
  int32_t* sorted_src;         // [n_targets]: ... and which of the user's targets each one is
  int32_t* user_unranked;      // [n_sel]
};

inline int64_t metric_workspace_bytes(int64_t n_sel, int64_t n_targets, int n_K) {
  return n_sel * (3 * n_K + 2) * 8 + n_targets * 8 + n_sel * 4;
}

__global__ __launch_bounds__(kPairBlock) void rank_metrics_users_kernel(MetricArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t s = int64_t(blockIdx.x) * (kPairBlock / 64) + (threadIdx.x >> 6);
  if (s >= a.n_sel) return;  // (the whole wavefront)
  const int nK = a.n_K, cols = 3 * nK + 2;
  double* out = a.user_vals + s * cols;
  // never outside the arrays, whatever the indptr holds (RFM_CHECK_IDS reports a bad one)
  const int64_t lo = min(max(a.tgt_indptr[s], int64_t(0)), a.n_targets);
  const int64_t hi = min(max(a.tgt_indptr[s + 1], lo), a.n_targets);

  int n_unranked = 0;
  long long rank_sum = 0;
  for (int64_t p0 = lo; p0 < hi; p0 += 64) {
    const int64_t p = p0 + lane;
    const int rp = p < hi ? a.ranks[p] : -1;
    int below = 0;
    for (int64_t q0 = lo; q0 < hi; q0 += 64) {
      const int rq = q0 + lane < hi ? a.ranks[q0 + lane] : -1;
      const int n = int(min(int64_t(64), hi - q0));
      for (int b = 0; b < n; ++b) {
        const int rb = lane_get(rq, b);
        below += int(rb >= 0 && (rb < rp || (rb == rp && q0 + b < p)));
      }
    }
    if (p < hi) {
      if (rp >= 0) {  // below < the number of ranked positives <= hi - lo
        a.sorted_rank[lo + below] = rp;
        a.sorted_src[lo + below] = int(p - lo);
        rank_sum += rp;
      } else {
        ++n_unranked;
      }
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    n_unranked += __shfl_xor(n_unranked, m, 64);
    rank_sum += __shfl_xor(rank_sum, m, 64);
  }
  if (lane == 0) a.user_unranked[s] = n_unranked;
  const int64_t P = (hi - lo) - n_unranked;
  if (P == 0) {  // no ranked positive: the user is in no mean
    if (lane < cols) out[lane] = NAN;
    return;
  }
  __threadfence_block();  // the ordered ranks were written by other lanes of this wavefront

  const int kind = lane / nK;  // 0 DCG, 1 Recall, 2 MAP; the lanes beyond add nothing
  const int64_t my_K = kind < 3 ? a.K[lane - kind * nK] : 0;
  double acc = 0.0;
  int r_first = 0;
  for (int64_t e0 = 0; e0 < P; e0 += 64) {
    const int64_t e = e0 + lane;
    const int re = e < P ? a.sorted_rank[lo + e] : 0x7fffffff;
    if (e0 == 0) r_first = lane_get(re, 0);
    if (int64_t(lane_get(re, 0)) >= a.max_K) break;  // ascending: no depth reaches the rest
    double t_dcg = 0.0, t_map = 0.0;
    if (e < P) {
      const double v = a.weights ? a.weights[lo + a.sorted_src[lo + e]] : 1.0;
      const double g = re == 0 ? 1.0 : 1.0 / log2(double(re) + 1.0);
      t_dcg = v * g;
      t_map = double(e + 1) / (double(re) + 1.0);
    }
    const int n = int(min(int64_t(64), P - e0));
    for (int b = 0; b < n; ++b) {
      const int r = lane_get(re, b);
      const double d = lane_get(t_dcg, b), m = lane_get(t_map, b);
      if (r < my_K) acc += kind == 0 ? d : kind == 1 ? 1.0 : m;
    }
  }
  if (lane < 3 * nK) out[lane] = kind == 1 ? acc / double(P) : acc;
  if (lane == 3 * nK) out[lane] = 1.0 / (double(r_first) + 1.0);
  if (lane == 3 * nK + 1) {
    const int64_t C = a.candidates[s];
    out[lane] = C > P ? 1.0 - double(rank_sum - P * (P - 1) / 2) / (double(P) * (double(C) - double(P))) : NAN;
  }
}

// Column blockIdx.x of the per-user table: the mean over the users whose value is not NaN (the
// host's nan-mean; a user that is not counted has NaN everywhere, a user with C <= P in the AUC
// column only), thread t adding users t, t + 256, ... and a fixed tree over the threads.
// counts[0] = users counted (the MRR column's), counts[1] = the AUC column's, counts[2] = unranked
// positives.
__global__ __launch_bounds__(kPairBlock) void rank_metrics_mean_kernel(
    const double* __restrict__ user_vals, const int32_t* __restrict__ user_unranked, int64_t n_sel,
    int n_K, double* __restrict__ out, int64_t* __restrict__ counts) {
  __shared__ double sv[kPairBlock];
  __shared__ long long sn[kPairBlock], su[kPairBlock];
  const int cols = 3 * n_K + 2, c = blockIdx.x, tid = threadIdx.x;
  double v = 0.0;
  long long n = 0, un = 0;
  for (int64_t s = tid; s < n_sel; s += kPairBlock) {
    const double x = user_vals[s * cols + c];
    if (x == x) {
      v += x;
      ++n;
    }
    if (c == 3 * n_K) un += user_unranked[s];
  }
  sv[tid] = v, sn[tid] = n, su[tid] = un;
  __syncthreads();
  for (int w = kPairBlock / 2; w >= 1; w >>= 1) {
    if (tid < w) sv[tid] += sv[tid + w], sn[tid] += sn[tid + w], su[tid] += su[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    out[c] = sv[0] / double(sn[0]);  // no user -> NaN
    if (c == 3 * n_K) counts[0] = sn[0], counts[2] = su[0];
    if (c == 3 * n_K + 1) counts[1] = sn[0];
  }
}

}  // namespace
}  // namespace rfm

using namespace rfm;

extern "C" {

int32_t rfm_fm_side_sums(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                         const double* d_values, int64_t n_rows, const double* d_w, const double* d_V,
                         int64_t n_features, int32_t n_factors, double* d_A, double* d_L) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_indptr && d_indices && d_values && d_w && d_V && d_A && d_L, "null pointer");
    RFM_REQUIRE(n_factors >= 1 && n_factors <= RFM_MAX_FACTORS, "n_factors=%d unsupported (1..%d)",
                n_factors, RFM_MAX_FACTORS);
    RFM_REQUIRE(n_rows >= 0 && n_features >= 1, "negative n_rows or no features");
    if (n_rows == 0) return;
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    IdCheck chk(ctx);
    const int64_t grid = (n_rows + kPairBlock / 64 - 1) / (kPairBlock / 64);
    RFM_REQUIRE(grid < (int64_t(1) << 31), "n_rows=%lld too large", (long long)n_rows);
    hipLaunchKernelGGL(side_sums_kernel, dim3((unsigned)grid), dim3(kPairBlock), 0, ctx->stream, d_indptr,
                       d_indices, d_values, n_rows, d_w, d_V, n_features, n_factors, int(pad4(n_factors)),
                       d_A, d_L, chk.flags());
    RFM_HIP_CHECK(hipGetLastError());
    chk.finish();
  });
}

int32_t rfm_pair_scores(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                        const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                        const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                        double* d_out) {
  return guarded([&] {
    PairArgs a = pair_args(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                           nullptr, nullptr);
    if (n_sel_users == 0) return;
    RFM_REQUIRE(d_out, "null output");
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    IdCheck chk(ctx);
    chk.begin(a);
    a.out = d_out;
    const dim3 grid((unsigned)((n_items + kTile - 1) / kTile), (unsigned)((n_sel_users + kTile - 1) / kTile));
    hipLaunchKernelGGL(pair_tile_kernel<kScores>, grid, dim3(kPairBlock), size_t(kOperandDoubles) * 8,
                       ctx->stream, a);
    RFM_HIP_CHECK(hipGetLastError());
    chk.finish();
  });
}

int32_t rfm_pair_topk_workspace(int64_t n_sel_users, int64_t n_items, int32_t k, int64_t* h_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_bytes, "null pointer");
    RFM_REQUIRE(k >= 1 && k <= kMaxTopK, "k=%d outside 1..%d", k, kMaxTopK);
    RFM_REQUIRE(n_sel_users >= 0 && n_items >= 1, "negative n_sel_users or no items");
    const Split sp = topk_split(n_sel_users, n_items);
    *h_bytes = std::max<int64_t>(16, int64_t(sp.n_splits) * n_sel_users * k * 12);
  });
}

int32_t rfm_pair_topk(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                      const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                      const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                      const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t k,
                      void* d_workspace, int32_t* d_out_items, double* d_out_scores) {
  return guarded([&] {
    pair_topk_run<false>(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                         d_excl_indptr, d_excl_items, k, d_workspace, d_out_items, d_out_scores);
  });
}

int32_t rfm_pair_topk_raw(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                          const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                          const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                          const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t k,
                          void* d_workspace, int32_t* d_out_items, double* d_out_values) {
  return guarded([&] {
    pair_topk_run<true>(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                        d_excl_indptr, d_excl_items, k, d_workspace, d_out_items, d_out_values);
  });
}

int32_t rfm_rows_normalise(rfm_ctx* ctx, const double* d_M, int64_t n_rows, int32_t n_factors, int64_t ld_in,
                           double* d_out, double* d_norm) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_M && d_out && d_norm, "null pointer");
    RFM_REQUIRE(n_factors >= 1 && n_factors <= RFM_MAX_FACTORS, "n_factors=%d unsupported (1..%d)",
                n_factors, RFM_MAX_FACTORS);
    RFM_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 40), "n_rows=%lld", (long long)n_rows);
    RFM_REQUIRE(ld_in >= n_factors && ld_in < (int64_t(1) << 20), "ld_in=%lld for %d factors", (long long)ld_in,
                n_factors);
    RFM_REQUIRE(d_out != d_M, "the rows cannot be normalised in place");
    if (n_rows == 0) return;
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    const bool wide = ld_in % 2 == 0 && reinterpret_cast<uintptr_t>(d_M) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    hipLaunchKernelGGL(rows_normalise_kernel, dim3(capped_grid(ctx, n_rows, kPairBlock / 64, 8, 1)),
                       dim3(kPairBlock), 0, ctx->stream, d_M, n_rows, n_factors, int(pad4(n_factors)), ld_in, wide,
                       d_out, d_norm);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_pair_ranks_workspace(int64_t n_sel_users, int64_t n_items, int64_t n_targets, int64_t* h_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_bytes, "null pointer");
    RFM_REQUIRE(n_sel_users >= 0 && n_items >= 1 && n_targets >= 0, "negative n_sel_users or n_targets, or no items");
    *h_bytes = std::max<int64_t>(16, n_targets * 8);  // the targets' logits
  });
}

int32_t rfm_pair_ranks(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                       const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                       const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                       const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                       const int64_t* d_tgt_indptr, const int32_t* d_tgt_items, void* d_workspace,
                       int32_t* d_out_ranks, double* d_out_scores, int32_t* d_out_candidates) {
  return guarded([&] {
    pair_ranks_run(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                   d_excl_indptr, d_excl_items, d_tgt_indptr, d_tgt_items, nullptr, d_workspace, d_out_ranks,
                   d_out_scores, d_out_candidates);
  });
}

int32_t rfm_pair_ranks_n(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                         const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                         const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                         const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                         const int64_t* d_tgt_indptr, const int32_t* d_tgt_items, int64_t n_targets,
                         void* d_workspace, int32_t* d_out_ranks, double* d_out_scores,
                         int32_t* d_out_candidates) {
  return guarded([&] {
    pair_ranks_run(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c,
                   d_excl_indptr, d_excl_items, d_tgt_indptr, d_tgt_items, &n_targets, d_workspace, d_out_ranks,
                   d_out_scores, d_out_candidates);
  });
}

int32_t rfm_rank_metrics_workspace(int64_t n_sel_users, int64_t n_targets, int32_t n_K, int64_t* h_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_bytes, "null pointer");
    RFM_REQUIRE(n_K >= 1 && n_K <= kMaxMetricK, "n_K=%d outside 1..%d", n_K, kMaxMetricK);
    RFM_REQUIRE(n_sel_users >= 0 && n_targets >= 0, "negative n_sel_users or n_targets");
    *h_bytes = std::max<int64_t>(16, metric_workspace_bytes(n_sel_users, n_targets, n_K));
  });
}

int32_t rfm_rank_metrics(rfm_ctx* ctx, const int64_t* d_tgt_indptr, int64_t n_sel_users, int64_t n_targets,
                         const int32_t* d_ranks, const int32_t* d_candidates, const double* d_weights,
                         const int64_t* h_K, int32_t n_K, void* d_workspace, double* d_out,
                         int64_t* d_out_counts) {
  return guarded([&] {
    RFM_REQUIRE(ctx && h_K && d_workspace && d_out && d_out_counts, "null pointer");
    RFM_REQUIRE(n_K >= 1 && n_K <= kMaxMetricK, "n_K=%d outside 1..%d", n_K, kMaxMetricK);
    RFM_REQUIRE(n_sel_users >= 0 && n_sel_users <= kMaxSel, "n_sel_users=%lld outside 0..%lld",
                (long long)n_sel_users, (long long)kMaxSel);
    RFM_REQUIRE(n_targets >= 0 && n_targets < (int64_t(1) << 40), "n_targets=%lld", (long long)n_targets);
    RFM_REQUIRE(n_sel_users == 0 || (d_tgt_indptr && d_candidates), "null target indptr or candidates");
    RFM_REQUIRE(n_targets == 0 || d_ranks, "null ranks");
    MetricArgs a{};
    a.n_K = n_K;
    for (int c = 0; c < n_K; ++c) {
      RFM_REQUIRE(h_K[c] >= 1, "K[%d]=%lld: a ranking depth must be at least 1", c, (long long)h_K[c]);
      a.K[c] = h_K[c];
      a.max_K = std::max(a.max_K, h_K[c]);
    }
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    IdCheck chk(ctx);
    if (n_sel_users > 0) chk.check_targets(d_tgt_indptr, nullptr, n_sel_users, 0, n_targets);
    a.tgt_indptr = d_tgt_indptr, a.ranks = d_ranks, a.candidates = d_candidates, a.weights = d_weights;
    a.n_sel = n_sel_users, a.n_targets = n_targets;
    const int cols = 3 * n_K + 2;
    a.user_vals = static_cast<double*>(d_workspace);
    a.sorted_rank = reinterpret_cast<int32_t*>(a.user_vals + n_sel_users * cols);
    a.sorted_src = a.sorted_rank + n_targets;
    a.user_unranked = a.sorted_src + n_targets;
    if (n_sel_users > 0) {
      const int64_t grid = (n_sel_users + kPairBlock / 64 - 1) / (kPairBlock / 64);
      hipLaunchKernelGGL(rank_metrics_users_kernel, dim3((unsigned)grid), dim3(kPairBlock), 0, ctx->stream, a);
      RFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(rank_metrics_mean_kernel, dim3((unsigned)cols), dim3(kPairBlock), 0, ctx->stream,
                       a.user_vals, a.user_unranked, n_sel_users, n_K, d_out, d_out_counts);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_pair_order_workspace(int64_t n_sel_users, int64_t n_items, int64_t depth, int64_t* h_min_bytes,
                                 int64_t* h_preferred_bytes) {
  return guarded([&] {
    RFM_REQUIRE(h_min_bytes && h_preferred_bytes, "null pointer");
    RFM_REQUIRE(depth >= 1, "depth=%lld: the ranking depth must be at least 1", (long long)depth);
    RFM_REQUIRE(n_sel_users >= 0 && n_items >= 1, "negative n_sel_users or no items");
    RFM_REQUIRE(n_items < (int64_t(1) << 31) - kTile, "n_items=%lld does not fit int32 item ids", (long long)n_items);
    *h_min_bytes = kTile * order_row_bytes(n_items);
    *h_preferred_bytes = std::max<int64_t>(1, (n_sel_users + kTile - 1) / kTile) * kTile * order_row_bytes(n_items);
  });
}

int32_t rfm_pair_geometry(int64_t n_sel_users, int64_t n_items, int32_t n_factors, int64_t* h_out8) {
  return guarded([&] {
    RFM_REQUIRE(h_out8, "null pointer");
    RFM_REQUIRE(n_factors >= 1 && n_factors <= RFM_MAX_FACTORS, "n_factors=%d unsupported (1..%d)",
                n_factors, RFM_MAX_FACTORS);
    RFM_REQUIRE(n_sel_users >= 1 && n_sel_users <= kMaxSel && n_items >= 1, "no selected user or no items");
    const int64_t kpad = pad4(n_factors);
    const int64_t chunks = (kpad + kChunk - 1) / kChunk;               // trips of the tile's k0 loop
    const int64_t k0 = (chunks - 1) * kChunk;                          // the last of them
    const int64_t item_tiles = (n_items + kTile - 1) / kTile;          // the tile's n_item_tiles
    const Split sp = topk_split(n_sel_users, n_items);
    h_out8[0] = kpad;
    h_out8[1] = chunks;
    h_out8[2] = std::min<int64_t>(kChunk, kpad - k0) >> 2;             // the tile's q at k0
    h_out8[3] = (n_sel_users + kTile - 1) / kTile;                     // grid y of every pair launch
    h_out8[4] = item_tiles;
    h_out8[5] = sp.n_splits;
    h_out8[6] = sp.tiles_per_split;
    // the tile's t_last - t_first of the last workgroup along x
    h_out8[7] = std::min<int64_t>(int64_t(sp.n_splits) * sp.tiles_per_split, item_tiles) -
                int64_t(sp.n_splits - 1) * sp.tiles_per_split;
  });
}

int32_t rfm_pair_order_geometry(int64_t n_items, int64_t depth, int64_t* h_out4) {
  return guarded([&] {
    RFM_REQUIRE(h_out4, "null pointer");
    RFM_REQUIRE(depth >= 1, "depth=%lld: the ranking depth must be at least 1", (long long)depth);
    RFM_REQUIRE(n_items >= 1 && n_items < (int64_t(1) << 31) - kTile, "n_items=%lld: none, or too many for int32 item ids",
                (long long)n_items);
    const int64_t n_ranks = std::min(depth, n_items);  // as rfm_pair_order
    const int P = order_list_len(n_ranks);
    h_out4[0] = P;
    h_out4[1] = order_pass(P);
    h_out4[2] = P - order_pass(P);           // a pass is preceded by a flush when more than this is staged
    h_out4[3] = (n_ranks + P - 1) / P;       // launches of the ranking kernel per block of users
  });
}

int32_t rfm_pair_order(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                       const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                       const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                       const int64_t* d_excl_indptr, const int32_t* d_excl_items, int64_t depth,
                       void* d_workspace, int64_t workspace_bytes, int32_t* d_out_items,
                       double* d_out_scores, int32_t* d_out_n_ranked) {
  return guarded([&] {
    pair_order_run(ctx, d_A, d_LU, n_users, d_user_ids, n_sel_users, d_B, d_LI, n_items, n_factors, d_c, d_excl_indptr,
                   d_excl_items, depth, d_workspace, workspace_bytes, d_out_items, d_out_scores, d_out_n_ranked);
  });
}

// The item -> users direction (include/rfm_audience.h): the twins' run functions in the by-item form.
int32_t rfm_pair_topk_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                              const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                              const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                              const int64_t* d_excl_indptr, const int32_t* d_excl_users, int32_t k, int32_t raw,
                              void* d_workspace, int32_t* d_out_users, double* d_out_values) {
  return guarded([&] {
    const auto run = raw ? pair_topk_run<true, kByItem> : pair_topk_run<false, kByItem>;
    run(ctx, d_A, d_LU, n_users, d_item_ids, n_sel_items, d_B, d_LI, n_items, n_factors, d_c, d_excl_indptr,
        d_excl_users, k, d_workspace, d_out_users, d_out_values);
  });
}

int32_t rfm_pair_ranks_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                               const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                               const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                               const int64_t* d_excl_indptr, const int32_t* d_excl_users,
                               const int64_t* d_tgt_indptr, const int32_t* d_tgt_users, int64_t n_targets,
                               void* d_workspace, int32_t* d_out_ranks, double* d_out_scores,
                               int32_t* d_out_candidates) {
  return guarded([&] {
    pair_ranks_run<kByItem>(ctx, d_A, d_LU, n_users, d_item_ids, n_sel_items, d_B, d_LI, n_items, n_factors, d_c,
                            d_excl_indptr, d_excl_users, d_tgt_indptr, d_tgt_users, &n_targets, d_workspace,
                            d_out_ranks, d_out_scores, d_out_candidates);
  });
}

int32_t rfm_pair_order_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                               const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                               const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                               const int64_t* d_excl_indptr, const int32_t* d_excl_users, int64_t depth,
                               void* d_workspace, int64_t workspace_bytes, int32_t* d_out_users,
                               double* d_out_scores, int32_t* d_out_n_ranked) {
  return guarded([&] {
    pair_order_run<kByItem>(ctx, d_A, d_LU, n_users, d_item_ids, n_sel_items, d_B, d_LI, n_items, n_factors, d_c,
                            d_excl_indptr, d_excl_users, depth, d_workspace, workspace_bytes, d_out_users,
                            d_out_scores, d_out_n_ranked);
  });
}

}  // extern "C"
