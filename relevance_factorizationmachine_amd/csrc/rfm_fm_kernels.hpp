// Device code of the FM path (gfx950).  See rfm_fm.hip for the launch side and
// DESIGN.md section 4 for the algorithm.  Reference arithmetic: src/fm.py:80-88,
// 114-187, src/base.py:37-66.
#pragma once

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rfm_common.h"
#include "rfm_device_utils.hpp"
#include "rfm_fm_records.h"
#include "rfm_rule.hpp"

namespace rfm {

// ---------------------------------------------------------------------------
// helpers (lane-group sums, packs, sigmoid: rfm_device_utils.hpp)
// ---------------------------------------------------------------------------
// fixed-order block sum (tree over LDS); every thread gets the total
template <int BLOCK>
__device__ inline double block_sum(double v, double* lds) {
  const int tid = threadIdx.x;
  __syncthreads();
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) lds[tid] += lds[tid + s];
    __syncthreads();
  }
  return lds[0];
}

__device__ inline double logloss_term(double y, double p, double pred, double eps) {
  const double r = y / p;
  return r * log(pred + eps) + (1.0 - r) * log(1.0 - pred + eps);
}

constexpr int kBigBlock = 1024;  // threads of the forward's many-rows-in-flight shape
constexpr int kSmallBlock = 256;  // threads of the one-row-per-group shape
// waves per SIMD the big forward shape is compiled for (register budget 512/N)
constexpr int kBigWaves = 4;
// rows per lane group of the big forward shape (single-chunk factor counts)
constexpr int kFwdRows = 2;

// entries of a row whose V gathers the one-row forward shape keeps in flight
constexpr int kBigUnroll = 3;
constexpr int kSmallUnroll = 8;
// ... of the one-row shape at two to four chunks of factors per lane (k = 300 / 400: an entry is
// NC gathers per lane; the shape runs about two waves per SIMD, so registers are not the limit)
constexpr int kSmallWideUnroll = 2;

// rows a lane group works on concurrently (independent load chains in flight)
constexpr int rows_in_flight(int nc) { return nc == 1 ? kFwdRows : 1; }
// ... of the PLAIN forward (the caller's CSR arrays: predict, validation loss), which keeps no Q
// row, leaves no marks and sums no hot class
constexpr int kFwdRowsPlain = kFwdRows;
constexpr int kPlainUnroll = kBigUnroll;
constexpr int rows_in_flight_plain(int nc) { return nc == 1 ? kFwdRowsPlain : 1; }

// Hot-class sums in a fixed order (training forward): the rows a workgroup holds in one trip
// leave their Q rows and per-entry coefficients in LDS, every hot column gets the set of those
// rows that hold it (a bitmap) and one lane group -- its owner -- adds them up in row order.
// Possible when a lane holds one chunk of factors and a trip is at most 128 rows; the other
// shapes add with LDS float atomics (arrival order).
constexpr bool hot_fixed_order(int lpr, int nc, int block, int rows) {
  return nc == 1 && (block / lpr) * rows <= 128;
}
// Hot tile (arrival-order hot sums, 16 lanes x 2 factors per row): the kTileRanks most frequent
// hot columns' err * x * q are summed on the matrix core, see the kernel's hot pass
constexpr int kTileRanks = 16;  // 16 or 32: tiles of 16 ranks (32 measured no faster: DESIGN.md section 7)
constexpr bool hot_tile(int lpr, int vec, int nc) { return lpr == 16 && vec == 2 && nc == 1; }
// The step's forward at 8 lanes x 2 chunks x 2 factors per row (fm_forward_lanes8): k = 20, 24, 28, 32
// on padded row blocks, many-rows shape, arrival-order hot sums.  The plan stays that of 16 lanes per row.
constexpr bool forward_lanes8(int k) { return k > 16 && k <= 32 && k % 4 == 0; }
constexpr int kHotUnroll = 2;  // rows of a fixed-order hot sum whose LDS reads are in flight together
constexpr int kHotPosPad = 4;  // bytes between the position rows of two columns (bank spread)

// The forms of fm_forward_kernel: where a row's entries come from, and what the launch does besides
// scoring its rows (the values are the C ABI's, rfm_fm_step_form).
enum class FwdKind : int {
  // the caller's CSR arrays (predict, validation loss): no Q rows, marks or hot class
  kCsr = RFM_FWD_CSR,
  // ... of two logs in one launch (many-rows shape): the train-loss and validation-loss forwards of a
  // fit() iteration, each part with its own loss partials -- see FwdArgs, n_rows_a
  kCsrPair = RFM_FWD_CSR_PAIR,
  // the training plan's records (RowRec / Entry)
  kRecords = RFM_FWD_RECORDS,
  // ... in their padded form, one row block Entry[LPR] per row (a.ell)
  kBlocks = RFM_FWD_BLOCKS,
  // records / blocks with the hot-class sums in a fixed order (hot_fixed_order) instead of LDS atomics
  kRecordsFixed = RFM_FWD_RECORDS_FIXED,
  kBlocksFixed = RFM_FWD_BLOCKS_FIXED,
  // records / blocks (one-row shape) with riding rows: the last workgroups only score rows of another
  // batch and of another log -- see FwdArgs, grid_main
  kRecordsRiders = RFM_FWD_RECORDS_RIDERS,
  kBlocksRiders = RFM_FWD_BLOCKS_RIDERS,
};
constexpr bool fwd_records(FwdKind k) { return k != FwdKind::kCsr && k != FwdKind::kCsrPair; }
constexpr bool fwd_blocks(FwdKind k) {
  return k == FwdKind::kBlocks || k == FwdKind::kBlocksFixed || k == FwdKind::kBlocksRiders;
}
constexpr bool fwd_fixed(FwdKind k) { return k == FwdKind::kRecordsFixed || k == FwdKind::kBlocksFixed; }
constexpr bool fwd_riders(FwdKind k) { return k == FwdKind::kRecordsRiders || k == FwdKind::kBlocksRiders; }
// rows a lane group of fm_forward_kernel keeps in flight
constexpr int forward_rows(int block, int nc, FwdKind kind) {
  return block != kBigBlock ? 1 : fwd_records(kind) ? rows_in_flight(nc) : rows_in_flight_plain(nc);
}
// the instantiations of fm_forward_kernel that are built
constexpr bool forward_form_exists(int lpr, int nc, int block, FwdKind kind) {
  if (block != kBigBlock && block != kSmallBlock) return false;
  if (kind == FwdKind::kCsrPair) return block == kBigBlock;
  if (fwd_riders(kind)) return block == kSmallBlock;
  if (fwd_fixed(kind)) return hot_fixed_order(lpr, nc, block, forward_rows(block, nc, kind));
  return true;
}
// Entries of a row whose V gathers fm_forward_kernel keeps in flight together.  One-row shape at one
// chunk of factors per lane: kSmallUnroll, it has registers to spare; at two to four chunks
// kSmallWideUnroll, beyond that 2.  The many-rows shape is at its register budget with two (x the rows
// of a lane group), except at one chunk on padded row blocks or the caller's CSR arrays with
// arrival-order hot sums, which hold three.
constexpr int gather_unroll(int block, int nc, FwdKind kind) {
  if (block != kBigBlock) return nc == 1 ? kSmallUnroll : nc > 4 ? 2 : kSmallWideUnroll;
  if (nc == 1 && !fwd_fixed(kind) && (fwd_blocks(kind) || !fwd_records(kind)))
    return fwd_records(kind) ? kBigUnroll : kPlainUnroll;
  return 2;
}

// What a forward launch is (rfm_fm.hip, forward_form): the one answer to "which form does it take".
struct FwdForm {
  Shape shape;   // lanes per row, factors per lane and chunks of the plan's map of the factor count
  int block;     // threads of a workgroup: kBigBlock (many rows in flight) or kSmallBlock (one row)
  int grid;      // workgroups that score the launch's own rows (riding rows add theirs)
  int rows;      // rows a lane group keeps in flight
  int trip;      // rows of a workgroup's trip
  int lanes;     // lanes per row of the kernel that runs: 8 for fm_forward_lanes8_kernel, else shape.lpr
  FwdKind kind;
  bool lanes8;   // fm_forward_lanes8_kernel, not fm_forward_kernel
  bool fixed;    // fixed-order hot sums
  size_t lds;    // dynamic LDS bytes (0 until the arguments are known)
};
// LDS bytes of the forward kernels (what a launch asks for).  The 8-lane kernel asks for what the
// 16-lane many-rows shape asks for on the same plan, whose trip it keeps: its row buffers (16 entries
// a lane group, groups one record apart) reach 1 KiB back into `red`, which nothing uses before the
// trips are over.
inline size_t forward_lds_bytes(const FwdForm& f, int n_hot, int k) {
  const int block = f.block, lpr = f.shape.lpr, vec = f.shape.vec, nc = f.shape.nc;
  const int rows = f.trip / (block / lpr);
  const bool fixed_order = f.fixed;
  size_t bytes = size_t(block) * 8 + (size_t(block) * rows + size_t(block / lpr)) * sizeof(Entry) +
                 size_t(n_hot) * size_t(k + 2) * 8;
  // (many-rows shape without a hot class -- the loss forwards: two stages of a trip's
  // {score, label, propensity}, see the kernel)
  if (block == kBigBlock && n_hot == 0) bytes += 2 * size_t(block / lpr) * rows * 24;
  // (hot tile: a lane group's coefficients by rank, one strip per row in flight)
  if (!fixed_order && n_hot > 0 && hot_tile(lpr, vec, nc))
    bytes += size_t(block / lpr) * rows * kTileRanks * 8;
  if (fixed_order && n_hot > 0 && hot_fixed_order(lpr, nc, block, rows)) {
    const size_t rt = size_t(block / lpr) * rows;
    bytes += rt * size_t(lpr * vec) * 8;                                 // Q rows of the trip
    if (rt / 32 > 1) bytes += size_t(block / lpr) * size_t(k + 2) * 8;   // cell sums
    bytes += ((size_t(n_hot) * ((rt + 31) / 32) + 1) & ~size_t(1)) * 4;  // row sets
    bytes += (size_t(n_hot) * (rt + kHotPosPad) + 7) / 8 * 8;            // entry positions
  }
  return bytes;
}

// ---------------------------------------------------------------------------
// 1. forward (+ residual, Q, slot marks, hot sums, loss partials)
// ---------------------------------------------------------------------------
struct FwdArgs {
  // the log: either the plan's records (training) ...
  const Entry* ent;
  const RowRec* rows;
  const char* ell;       // ... in their padded form when every row fits one round: row blocks
  int64_t ell_stride;    //     Entry[LPR] of this many bytes (then ent / rows are null), with
  const double2* ell_yp; //     the rows' {label, propensity} pairs (one line per row)
  // ... or the caller's CSR arrays (+ labels / propensities when a loss is asked for)
  const int64_t* indptr;
  const int32_t* indices;
  const double* values;
  const double* y;
  const double* pscore;
  const int32_t* row_ids;  // may be null: row t
  int64_t n_rows;
  // FwdKind::kCsrPair (loss forwards of fit(), caller's CSR arrays): rows [0, n_rows_a) are rows row_ids[t]
  // of the log above, rows [n_rows_a, n_rows) are rows t - n_rows_a of a SECOND log; each part
  // has its own loss partials -- the train-loss and validation-loss forwards in one launch
  int64_t n_rows_a;
  const int64_t* indptr2;
  const int32_t* indices2;
  const double* values2;
  const double* y2;
  const double* pscore2;
  double* loss_partial2;
  const double* w0;
  const double* w;
  const double* V;
  int32_t k;
  double* out_pred;      // nullable
  double* out_err;       // nullable
  double* out_Q;         // nullable [n_rows][k]
  SlotMark* slot_mark;   // nullable: leave {t, residual} at the slot of every sparse-class entry ...
  unsigned long long* slot_bits;  // ... and set the slot's bit (what fm_consume_kernel scans)
  int32_t n_hot;         // hot columns (training step only)
  int32_t hot_rounds;    // rounds of LPR entries that cover the longest row of the plan
  int32_t hot_fixed;     // 1: the plan asks for fixed-order hot sums (the ...Fixed kinds)
  double* hot_slab;      // [n_hot][gridDim.x][k+2]
  double* err_partial;   // nullable: [gridDim.x] per-workgroup sums of the residual (for w0)
  double* loss_partial;  // nullable: [gridDim.x]
  double eps;
  // The ...Riders kinds (one-row shape): workgroups grid_main .. gridDim.x - 1 only SCORE the rows
  // row_ids_x[0 .. n_rows_x) of the same plan (-> out_pred_x) -- no Q rows, marks, hot sums or
  // residuals: the train-loss forward of the previous batch, which reads the same parameters as
  // this step's forward, rides in its launch (rfm_fm_train)
  int32_t grid_main;
  const int32_t* row_ids_x;
  int64_t n_rows_x;
  double* out_pred_x;
  // ... and, after grid_x of those, workgroups that score EVERY row of another log given as row and
  // entry records (the validation log: rfm_fm_plan_register_log) -> out_pred_y
  int32_t grid_x;
  const RowRec* rows_y;
  const Entry* ent_y;
  int64_t n_rows_y;
  double* out_pred_y;
};

// what the arrival-order hot pass leaves in place of an entry record (16 B): the offset of the
// entry's column in the hot sums (-1: no add) and err * x
struct HotEnt {
  int32_t off;
  int32_t pad;
  double coef;
};
static_assert(sizeof(HotEnt) == sizeof(Entry), "HotEnt replaces an Entry in place");

// The step's forward at 8 lanes x 4 factors per row and ONE row per lane group (forward_lanes8;
// fm_forward_lanes8_kernel): the many-rows shape on padded row blocks
// with arrival-order hot sums, with fewer of the instructions of a row that do not depend on the
// factor -- addresses, parked-entry reads, scores, marks, walk bookkeeping serve 8 rows per
// wavefront instruction and are issued once, not once per row in flight.  Lane L of a group holds
// the factor pairs 2L, 2L + 1 and 16 + 2L, 16 + 2L + 1 -- lanes L and 8 + L of the 16-lane map, two
// chunks of 8 lanes x 2 factors -- so that each of its two 16-byte loads of a row of V is, over
// the group, one whole 128-byte line (four adjacent factors per lane touch every line twice, half
// of it each time: measured 1.2 us SLOWER than the 16-lane map).  It holds
// entries 2L, 2L + 1 of the row's block of 16.  Lane groups 2G and 2G + 1 -- one 16-lane slice --
// take the rows G and GPB / 2 + G of the trip, the two rows of group G of the 16-lane map.
//
// Every row comes out with the bits of the 16-lane map: a factor's sum runs over the entries in
// their order; a lane's two squared-sum partials go through group_sum<8> apart (stages l ^ 1,
// l ^ 2 and the half mirror of the 16-lane tree) and are added last (its row mirror); a lane's
// two linear terms are added first (stage l ^ 1), then group_sum<8> makes the other three stages;
// the slice's two residuals enter the workgroup's sum in the 16-lane map's thread and order.  The
// fused multiply-adds are spelled out where the 16-lane map's are contracted.
// LDS: as forward_lds_bytes says -- red | row buffers [GPB][16 + 1] Entry, ending where the
// 16-lane shape's end | hot sums [H][k+2] | coefficient strips [GPB][kTileRanks].
template <int BLOCK>
__device__ inline void fm_forward_lanes8(const FwdArgs& a) {
  constexpr int LPR = 8, VEC = 4, EPR = 16;  // lanes, factors of a lane, entries of a row block
  constexpr int GPB = BLOCK / LPR, GPW = kWave / LPR;
  static_assert(kTileRanks == 16 && EPR == 2 * LPR, "one tile of 16 ranks; two entries per lane");
  static_assert(GPB * (EPR + 1) <= BLOCK * kFwdRows + BLOCK / 16 + BLOCK / 16, "row buffers reach at most 1 KiB into red");
  extern __shared__ double dyn_lds[];
  const int tid = threadIdx.x;
  const int l = tid % LPR;
  const int g = tid / LPR;
  const int k = a.k;
  const int hot_w = k + 2;
  const int H = a.n_hot;
  const unsigned bx = blockIdx.x, gx = gridDim.x;
  double* red = dyn_lds;
  double* hot = dyn_lds + BLOCK + 2 * (BLOCK * kFwdRows + BLOCK / 16);
  Entry* ebuf = reinterpret_cast<Entry*>(hot) - (GPB - g) * (EPR + 1);
  const int rt = (g & 1) * (GPB / 2) + (g >> 1);  // the group's row of a trip
  const double w0 = a.w0[0];
  const int64_t last_row = a.n_rows - 1;
  double err_acc = 0.0;
  // the lane's two pairs of factors; a pair past k reads offset 0 and is masked
  const int f0 = 2 * l, f1 = 16 + 2 * l;
  const bool fok[2] = {true, f1 < k};  // (k > 16: the first pair is always there)
  const int fo[2] = {fok[0] ? f0 : 0, fok[1] ? f1 : 0};

  if (H > 0) {
    for (int i = tid; i < H * hot_w; i += BLOCK) hot[i] = 0.0;
    __syncthreads();
  }
  for (int64_t base = int64_t(bx) * GPB; base < a.n_rows; base += int64_t(gx) * GPB) {
    const int64_t t = base + rt;
    const bool valid = t <= last_row;
    int32_t r = int32_t(valid ? t : last_row);
    if (a.row_ids) r = a.row_ids[r];
    // the workgroup's next trip: its row id now and (under the hot pass) a touch of its row block
    const int64_t nbase = base + int64_t(gx) * GPB;
    const bool warm = a.row_ids && nbase < a.n_rows;
    int32_t nxt = 0;
    if (warm) nxt = a.row_ids[nbase + rt <= last_row ? nbase + rt : last_row];
    Entry e[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) e[n] = reinterpret_cast<const Entry*>(a.ell + int64_t(r) * a.ell_stride)[2 * l + n];
    const double2 yp = a.ell_yp[r];
    // the row's length: its entries that are not padding (they come first)
    int len = 0;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const unsigned long long live = __ballot(e[n].slot != kNilSlot);
      len += __popc(unsigned(live >> ((g % GPW) * LPR)) & ((1u << LPR) - 1u));
    }
    if (!valid) len = 0;
    double lin = 0.0;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (2 * l + n >= len) {  // padding: the row's own last entry again, with x = 0
        e[n].slot = 0;
        e[n].x = 0.0;
      }
      const double term = __builtin_fma(a.w[e[n].col], e[n].x, 0.0);
      lin = n == 0 ? term : lin + term;
      ebuf[2 * l + n] = e[n];
    }

    double q[VEC], s2[2];
#pragma unroll
    for (int v = 0; v < VEC; ++v) q[v] = 0.0;
    s2[0] = s2[1] = 0.0;
#pragma unroll(kBigUnroll)
    for (int j = 0; j < len; ++j) {
      const Entry ej = ebuf[j];  // same address in the lane group: broadcast
      const double* vrow = a.V + int64_t(ej.col) * k;
      Pack<2> pv[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) pv[n].load(vrow + fo[n]);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        // (a pair past k re-reads the head of a row of V the row holds anyway, times zero)
        const double xm = fok[n] ? ej.x : 0.0;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const double vx = pv[n].v[v] * xm;
          q[2 * n + v] = __builtin_fma(pv[n].v[v], xm, q[2 * n + v]);
          s2[n] = __builtin_fma(vx, vx, s2[n]);
        }
      }
    }

    // (the labels are in registers on every path from here, see fm_forward_kernel)
    asm volatile("" ::"v"(yp.x), "v"(yp.y));
    if (len == 0) {  // an empty row scores sigmoid(w0) whatever its padding holds
      s2[0] = s2[1] = 0.0;
      lin = 0.0;
#pragma unroll
      for (int v = 0; v < VEC; ++v) q[v] = 0.0;
    }
    double half[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
      half[n] = __builtin_fma(q[2 * n + 1], q[2 * n + 1], __builtin_fma(q[2 * n], q[2 * n], -s2[n]));
    const double pair = group_sum<LPR>(half[0]) + group_sum<LPR>(half[1]);
    const double linsum = group_sum<LPR>(lin);
    const double pred = sigmoid_clipped(w0 + linsum + 0.5 * pair);
    const double err = valid ? yp.x / yp.y - pred : 0.0;
    if (valid) {
      if (a.out_Q) {  // (Q belongs to a plan: max_batch * k fits 31 bits)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (fok[n]) {
            Pack<2> pq;
            pq.v[0] = q[2 * n];
            pq.v[1] = q[2 * n + 1];
            pq.store_through(a.out_Q + (uint32_t(t) * uint32_t(k) + uint32_t(fo[n])));
          }
        }
      }
      if (l == 0) {
        if (a.out_pred) a.out_pred[t] = pred;
        if (a.out_err) a.out_err[t] = err;
      }
    }
    {
      // the slice's two residuals by its first lane, in the order of the 16-lane map's thread
      const double second = dpp_across_8(err);
      if (tid % 16 == 0) {
        err_acc += err;
        err_acc += second;
      }
    }

    int32_t touched = 0;
    if (warm)  // lane l touches the 32 bytes of its own entries
      touched = *reinterpret_cast<const int32_t*>(a.ell + int64_t(nxt) * a.ell_stride + 32 * l);
    if (a.slot_mark || H > 0) {
      // after the residual is known: marks of the sparse-class entries, and the hot entries'
      // err * x * [q, 1, x] into the workgroup's LDS sums (see fm_forward_kernel's hot tile)
      Entry em[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) em[n] = ebuf[2 * l + n];
      if (a.slot_mark) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (2 * l + n < len && em[n].slot >= 0) {
            Pack<2> pm;
            pm.v[0] = __hiloint2double(0, int32_t(t));
            pm.v[1] = err;
            pm.store_through(reinterpret_cast<double*>(a.slot_mark + em[n].slot));
            atomicOr(a.slot_bits + (em[n].slot >> 6), 1ull << (em[n].slot & 63));
          }
        }
      }
      if (H > 0) {  // (uniform: the matrix core ignores the execution mask)
        typedef double tile_acc __attribute__((ext_vector_type(4)));
        int tid_here = tid;  // (the pass's lane constants are not hoisted over the gathers)
        asm volatile("" : "+v"(tid_here));
        const int lh = tid_here % LPR, gh = tid_here / LPR, gw = gh % GPW;
        const int l16 = tid_here % 16, slice = (tid_here % kWave) / 16;
        const bool upper = (tid_here & LPR) != 0;  // the second row of its 16-lane slice
        HotEnt* const hbuf = reinterpret_cast<HotEnt*>(ebuf);
        double* const strip = hot + H * hot_w;  // [GPB][kTileRanks], behind the hot sums
        // a row that is not valid, or whose residual is not finite, gives zeros to the tile and
        // keeps all its hot entries on the walk (containment of a non-finite row of V)
        const bool rowok = valid && __builtin_isfinite(err);
        double* const st = strip + gh * kTileRanks;
        Pack<2> zero;
        zero.v[0] = zero.v[1] = 0.0;
        zero.store(st + 2 * lh);
        bool won[2];
        unsigned long long walked[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const bool live = 2 * l + n < len && em[n].slot < 0;
          const int h = -1 - em[n].slot;
          const bool tile_e = live && rowok && h < kTileRanks;
          won[n] = live && !tile_e;
          walked[n] = __ballot(won[n]);
          const double coef = err * em[n].x;
          if (live) {  // the [k] / [k+1] sums by the entry's own lane, tile entry or not
            double* const hsum = hot + (-em[n].slot * hot_w - 2);
            unsafeAtomicAdd(hsum, coef);
            unsafeAtomicAdd(hsum + 1, coef * em[n].x);
          }
          if (tile_e) st[h] = coef;  // (after the zeros: same wavefront, program order)
        }
        // the entries the wave walks: the largest count of a row of its groups (scalar)
        int wcnt = 0;
#pragma unroll
        for (int gq = 0; gq < GPW; ++gq)
          wcnt = max(wcnt, __popc(unsigned(walked[0] >> (gq * LPR)) & ((1u << LPR) - 1u)) +
                               __popc(unsigned(walked[1] >> (gq * LPR)) & ((1u << LPR) - 1u)));
        const int rot = (gw * wcnt) / GPW;  // (the groups of a wave start at different entries)
        {
          // walked entries first -- the lanes' first entries, then their second ones -- and the
          // others behind them as fillers
          const unsigned b0 = unsigned(walked[0] >> (gw * LPR)) & ((1u << LPR) - 1u);
          const unsigned b1 = unsigned(walked[1] >> (gw * LPR)) & ((1u << LPR) - 1u);
          const unsigned lower = (1u << lh) - 1u;
          const int n0 = __popc(b0), nw = n0 + __popc(b1);
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const int below = n == 0 ? __popc(b0 & lower) : n0 + __popc(b1 & lower);
            const int p = won[n] ? below : nw + n * LPR + lh - below;
            const int at = p - rot < 0 ? p - rot + wcnt : p - rot;
            if (p < wcnt)
              hbuf[at] = HotEnt{won[n] ? (-1 - em[n].slot) * hot_w : -1, 0, err * em[n].x};
          }
        }
        // G[rank][factor] += C[rank][row] * Q[row][factor] on the matrix core.  A K index is one
        // row: the first rows of the wave's four slices in one product, the second rows in the
        // next.  Column j < 8 of a product is factor 16 vp + 2 j, column 8 + j factor 16 vp + 2 j + 1
        // (vp: the factor pair of a lane), so a lane of the row's own group gives one of its
        // factors as it stands and its neighbour 8 lanes away passes on the other.
        const double c0 = strip[(gh & ~1) * kTileRanks + l16];
        const double c1 = strip[(gh | 1) * kTileRanks + l16];
#pragma unroll
        for (int vp = 0; vp < VEC / 2; ++vp) {
          const double even = rowok ? q[2 * vp] : 0.0, odd = rowok ? q[2 * vp + 1] : 0.0;
          const double odd_across = dpp_across_8(odd), even_across = dpp_across_8(even);
          const double b0 = upper ? odd_across : even;   // the slice's first row
          const double b1 = upper ? odd : even_across;   // its second row
          tile_acc D = tile_acc{0.0, 0.0, 0.0, 0.0};
          D = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, b0, D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, b1, D, 0, 0, 0);
          // flush: D register `reg` of a lane is rank (lane >> 4) + 4 reg, column lane & 15
          const int f = 16 * vp + 2 * (l16 % LPR) + (upper ? 1 : 0);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int rank = slice + 4 * reg;
            if (rank < H && f < k) unsafeAtomicAdd(hot + rank * hot_w + f, D[reg]);
          }
        }
        for (int j = 0; j < wcnt; ++j) {
          const HotEnt eh = hbuf[j];  // broadcast in the group
          if (eh.off >= 0) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              if (fok[n]) {
                double* hrow = hot + eh.off + fo[n];
#pragma unroll
                for (int v = 0; v < 2; ++v) unsafeAtomicAdd(hrow + v, eh.coef * q[2 * n + v]);
              }
            }
          }
        }
      }
    }
    if (warm) asm volatile("" ::"v"(touched));  // keep the touch alive
  }

  if (H > 0) {
    __syncthreads();
    // slab layout [H][gridDim.x][k+2], rows of whole 16-byte pairs written through (the gradient
    // launch reads the slabs next)
    for (int i = 2 * tid; i < H * hot_w; i += 2 * BLOCK) {
      const int h = i / hot_w, f = i % hot_w;
      Pack<2> ps;
      ps.load(hot + i);
      ps.store_through(a.hot_slab + (int64_t(h) * gx + bx) * hot_w + f);
    }
  }
  if (a.err_partial) {
    const double s = block_sum<BLOCK>(err_acc, red);
    if (tid == 0) a.err_partial[bx] = s;
  }
}

// the 8-lane step forward's entry: launched in place of fm_forward_kernel<16, 2, 1, kBigBlock, kBlocks>
template <int BLOCK>
__global__ __launch_bounds__(BLOCK, (BLOCK == kBigBlock ? kBigWaves : 1)) void fm_forward_lanes8_kernel(
    FwdArgs a) {
  fm_forward_lanes8<BLOCK>(a);
}

// A row is handled by LPR consecutive lanes; lane l holds factors
// (c*LPR + l)*VEC .. +VEC-1 for c < NC.  k=32 -> LPR=16, VEC=2: one 16-byte
// load per lane covers a 256-byte row of V, four rows per wave.
//
// One batch is only a few hundred rows per CU, so the kernel is bound by the
// latency of the chain row id -> row record -> entries -> V rows, not by bytes.
// Hence: a lane group keeps R rows in flight; the R x LPR entry records of a
// round are loaded once (one per lane), parked in LDS and re-read as 16-byte
// broadcasts (no cross-lane shuffles); and NO load sits under a divergent
// branch -- indices are clamped and results masked instead -- so that the
// loads of the R rows and of consecutive entries are issued back to back
// rather than each waiting for the previous one.
//
// K: the form, see FwdKind; forward_form_exists says which are built.
// LDS (dynamic): red[BLOCK] f64 | entry buffer [BLOCK/LPR][R*LPR+1] Entry | hot sums [H][k+2] f64
//   | hot tile: coefficient strips [R][BLOCK/LPR][kTileRanks] f64 (hot_tile shapes, REC && !DET)
//   | fixed-order hot sums (DET): Q rows, cell sums, row sets, entry positions
template <int LPR, int VEC, int NC, int BLOCK, FwdKind K>
__global__ __launch_bounds__(BLOCK, (BLOCK == kBigBlock ? kBigWaves : 1)) void fm_forward_kernel(
    FwdArgs a) {
  static_assert(forward_form_exists(LPR, NC, BLOCK, K), "this form of the forward is not built");
  constexpr bool REC = fwd_records(K);            // the plan's records, not the caller's CSR arrays
  constexpr bool ELL = fwd_blocks(K);             // ... as padded row blocks
  constexpr bool DET = fwd_fixed(K);              // fixed-order hot sums
  constexpr bool SEG = K == FwdKind::kCsrPair;    // two logs in one launch
  constexpr bool XTRA = fwd_riders(K);            // riding rows
  constexpr int R = forward_rows(BLOCK, NC, K);   // rows a lane group keeps in flight
  constexpr int GPB = BLOCK / LPR;  // lane groups per block
  // workgroup index and count among the workgroups of its kind (XTRA: the step's, or the ones
  // that only score the extra rows -- a workgroup-uniform switch of what the arguments mean)
  unsigned bx = blockIdx.x, gx = gridDim.x;
  if constexpr (XTRA && REC) {
    if (int(blockIdx.x) >= a.grid_main) {
      const bool second = int(blockIdx.x) >= a.grid_main + a.grid_x;
      bx = blockIdx.x - a.grid_main - (second ? a.grid_x : 0);
      gx = second ? gridDim.x - a.grid_main - a.grid_x : a.grid_x;
      a.row_ids = second ? nullptr : a.row_ids_x;
      a.n_rows = second ? a.n_rows_y : a.n_rows_x;
      if (second) {
        a.rows = a.rows_y;
        a.ent = a.ent_y;
      }
      a.n_hot = 0;
      a.slot_mark = nullptr;
      a.slot_bits = nullptr;
      a.out_Q = nullptr;
      a.out_err = nullptr;
      a.err_partial = nullptr;
      a.loss_partial = nullptr;
      a.out_pred = second ? a.out_pred_y : a.out_pred_x;
    } else {
      gx = a.grid_main;
    }
  }
  constexpr bool seg = SEG && !REC;
  extern __shared__ double dyn_lds[];
  const int tid = threadIdx.x;
  const int l = tid % LPR;
  const int g = tid / LPR;
  const int k = a.k;
  const int hot_w = k + 2;
  const int H = a.n_hot;
  double* red = dyn_lds;
  // this group's [R][LPR] entry records; groups are one record apart in bank space so that
  // the broadcast reads of different groups do not collide
  Entry* ebuf = reinterpret_cast<Entry*>(dyn_lds + BLOCK) + g * (R * LPR + 1);
  double* hot = dyn_lds + BLOCK + 2 * (BLOCK * R + GPB);
  // fixed-order hot sums (see hot_fixed_order): Q rows | row sets | entry positions
  constexpr bool FIX = DET && REC && hot_fixed_order(LPR, NC, BLOCK, R);
  constexpr int RT = GPB * R;            // rows of a trip
  constexpr int KS = LPR * VEC;          // doubles of a parked Q row
  constexpr int NW = (RT + 31) / 32;     // 32-bit words of a column's row set
  constexpr int NCELL = RT / 32 > 1 ? RT / 32 : 1;  // cells (32 rows) a frequent column is cut into
  constexpr int NHV = NCELL > 1 ? GPB / NCELL : 0;  // columns cut into cells: one cell per group
  constexpr int PS = RT + kHotPosPad;    // bytes of a column's position row
  double* Qs = hot + H * hot_w;
  // hot tile (see the arrival-order hot pass): the kTileRanks most frequent hot columns' factor
  // sums go through the matrix core
  constexpr bool TILE = REC && !DET && hot_tile(LPR, VEC, NC);
  double* part = Qs + RT * KS;           // [GPB][k+2] cell sums (NCELL > 1)
  unsigned int* hbits = reinterpret_cast<unsigned int*>(part + (NCELL > 1 ? GPB * hot_w : 0));
  uint8_t* hpos = reinterpret_cast<uint8_t*>(hbits + ((H * NW + 1) & ~1));
  const double w0 = a.w0[0];
  const int64_t last_row = a.n_rows - 1;
  double loss_acc = 0.0, loss_acc2 = 0.0, err_acc = 0.0;
  // many-rows shape, loss asked for, no hot class (whose sums would sit where the stages do)
  const bool stage_loss = BLOCK == kBigBlock && a.loss_partial != nullptr && H == 0;
  double* lstage = hot;  // [2][RT][3]
  int trip = 0;
  // factor offsets of this lane; lanes past k read offset 0 and are masked
  int fo[NC];
  bool fok[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * LPR + l) * VEC;
    fok[c] = f < k;
    fo[c] = fok[c] ? f : 0;
  }

  if (H > 0) {
    for (int i = tid; i < H * hot_w; i += BLOCK) hot[i] = 0.0;
    if (FIX)
      for (int i = tid; i < H * NW; i += BLOCK) hbits[i] = 0u;
    __syncthreads();
  }
  for (int64_t base = int64_t(bx) * (GPB * R); base < a.n_rows;
       base += int64_t(gx) * (GPB * R)) {
    int64_t t[R];
    int32_t r[R];  // rows of a log (or of a batch) fit 31 bits
    // entry offsets: the plan checks that they fit 31 bits; the caller's CSR is taken as it is
    using EntryOff = typename std::conditional<REC, int32_t, int64_t>::type;
    EntryOff p0[R];
    int len[R];
    double yy[R], pp[R];
    bool valid[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      t[i] = base + i * GPB + g;
      valid[i] = t[i] <= last_row;
      r[i] = int32_t(valid[i] ? t[i] : last_row);
    }
    bool sb[R];  // SEG: the row belongs to the second log
#pragma unroll
    for (int i = 0; i < R; ++i) sb[i] = seg && (valid[i] ? t[i] : last_row) >= a.n_rows_a;
    if (a.row_ids) {  // uniform: the R loads stay in one block and overlap
#pragma unroll
      for (int i = 0; i < R; ++i) r[i] = a.row_ids[sb[i] ? 0 : r[i]];
    }
    if constexpr (seg) {
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (sb[i]) r[i] = int32_t((valid[i] ? t[i] : last_row) - a.n_rows_a);
    }
    // the workgroup's NEXT trip: its row ids now, and (below, under the hot pass) a touch of
    // its row blocks, so that the next trip's first two dependent loads find their lines
    // on chip instead of waiting for memory
    int32_t nxt[R];
    const int64_t nbase = base + int64_t(gx) * (GPB * R);
    constexpr bool ell = REC && ELL;
    const bool warm = ell && BLOCK == kBigBlock && a.row_ids && nbase < a.n_rows;
    int32_t* parked = reinterpret_cast<int32_t*>(red);  // (red is only used after the trips)
    if (warm) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int64_t nt = nbase + i * GPB + g;
        nxt[i] = a.row_ids[nt <= last_row ? nt : last_row];
      }
    }
    Entry e0[R];  // ell: the row's entry of this lane, loaded next to the row's head
    if (ell) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        e0[i] = reinterpret_cast<const Entry*>(a.ell + int64_t(r[i]) * a.ell_stride)[l];
        const double2 yp = a.ell_yp[r[i]];
        yy[i] = yp.x;
        pp[i] = yp.y;
        p0[i] = 0;
      }
      // the row's length: its entries that are not padding (they come first)
      constexpr int GPW = kWave / LPR;  // lane groups of a wave
#pragma unroll
      for (int i = 0; i < R; ++i) {
        unsigned long long live = __ballot(e0[i].slot != kNilSlot);
        if (GPW > 1) live = (live >> ((g % GPW) * LPR)) & ((1ull << (LPR % 64)) - 1ull);
        len[i] = valid[i] ? __popcll(live) : 0;
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (ell) {
      } else if (REC) {
        const RowRec rec = a.rows[r[i]];
        p0[i] = EntryOff(rec.begin);
        len[i] = valid[i] ? int(rec.len) : 0;
        yy[i] = rec.y;
        pp[i] = rec.p;
      } else {
        const int64_t* ip = sb[i] ? a.indptr2 : a.indptr;
        const int64_t b0 = ip[r[i]], b1 = ip[r[i] + 1];
        p0[i] = EntryOff(b0);
        len[i] = valid[i] ? int(b1 - b0) : 0;
        yy[i] = 0.0;
        pp[i] = 1.0;
      }
    }
    if (!REC && a.y) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        yy[i] = (sb[i] ? a.y2 : a.y)[r[i]];
        pp[i] = (sb[i] ? a.pscore2 : a.pscore)[r[i]];
      }
    }
    int maxlen = len[0];
#pragma unroll
    for (int i = 1; i < R; ++i) maxlen = max(maxlen, len[i]);
    if (warm) {
      // the next trip's ids arrived with this trip's heads; they wait in LDS while the
      // gathers need every register
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (l == 0) parked[i * GPB + g] = nxt[i];
    }

    double q[R][NC][VEC];
    double s2[R], lin[R], err[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      s2[i] = 0.0;
      lin[i] = 0.0;
      err[i] = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) q[i][c][v] = 0.0;
    }

    for (int pb = 0; pb < maxlen; pb += LPR) {
      // stage this round's entries: one per lane and row (padding: column 0, x = 0)
      Entry e[R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int my = pb + l;
        // clamp into the row's own entries (entry 0 of the log for an empty row)
        const EntryOff at = len[i] > 0 ? p0[i] + min(my, len[i] - 1) : 0;
        if (ell) {
          e[i] = e0[i];  // one round; the block is padded with the row's last entry
        } else if (REC) {
          e[i] = a.ent[at];
        } else {
          e[i].col = (sb[i] ? a.indices2 : a.indices)[at];
          e[i].slot = 0;
          e[i].x = (sb[i] ? a.values2 : a.values)[at];
        }
        // padding: the row's own last entry again with x = 0 (not some fixed column: a
        // non-finite row of V must reach only the rows that hold its column; an empty
        // row, whose padding is entry 0 of the log, has its sums cleared below)
        if (my >= len[i]) {
          e[i].slot = 0;
          e[i].x = 0.0;
        }
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        lin[i] += a.w[e[i].col] * e[i].x;
        ebuf[i * LPR + l] = e[i];
      }
      const int cnt = (maxlen - pb) < LPR ? (maxlen - pb) : LPR;
      // entries whose gathers are in flight together
#pragma unroll gather_unroll(BLOCK, NC, K)
      for (int j = 0; j < cnt; ++j) {
        Entry ej[R];
        Pack<VEC> pv[R][NC];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          ej[i] = ebuf[i * LPR + j];  // same address in the lane group: broadcast
          const double* vrow = a.V + int64_t(ej[i].col) * k;
#pragma unroll
          for (int c = 0; c < NC; ++c) pv[i][c].load(vrow + fo[c]);
        }
        // padding entries carry x = 0 and lanes past k get a zero multiplier (both re-read
        // values of a column the row holds anyway): the products vanish without a select
        // or branch, so the gathers above stay unconditional and in flight together
#pragma unroll
        for (int i = 0; i < R; ++i) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const double xm = fok[c] ? ej[i].x : 0.0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              const double vx = pv[i][c].v[v] * xm;
              q[i][c][v] += vx;
              s2[i] += vx * vx;
            }
          }
        }
      }
    }

    if (warm) {  // back from LDS (same wave wrote them): the gathers' registers are free again
#pragma unroll
      for (int i = 0; i < R; ++i) nxt[i] = parked[i * GPB + g];
    }
    // the labels are in registers on every path from here: a path that leaves their loads
    // pending makes the compiler drain ALL memory operations (the next trip's touches, the
    // marks) with a vmcnt(0) in the hot pass, before it rewrites their registers
#pragma unroll
    for (int i = 0; i < R; ++i) asm volatile("" ::"v"(yy[i]), "v"(pp[i]));
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (len[i] == 0) {  // an empty row scores sigmoid(w0) whatever its padding gathered
        s2[i] = 0.0;
        lin[i] = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) q[i][c][v] = 0.0;
      }
      double pair = -s2[i];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) pair += q[i][c][v] * q[i][c][v];
      pair = group_sum<LPR>(pair);
      const double linsum = group_sum<LPR>(lin[i]);
      const double pred = sigmoid_clipped(w0 + linsum + 0.5 * pair);
      err[i] = valid[i] ? yy[i] / pp[i] - pred : 0.0;
      if (valid[i]) {
        if (a.out_Q) {
          // (Q belongs to a plan: max_batch * k fits 31 bits, checked where it is made)
          const uint32_t qoff = uint32_t(t[i]) * uint32_t(k);
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (fok[c]) {
              Pack<VEC> pq;
#pragma unroll
              for (int v = 0; v < VEC; ++v) pq.v[v] = q[i][c][v];
              // (training: the gradient launch reads the row next, nothing here does)
              if (REC)
                pq.store_through(a.out_Q + (qoff + uint32_t(fo[c])));
              else
                pq.store(a.out_Q + (qoff + uint32_t(fo[c])));
            }
          }
        }
        if (l == 0) {
          if (a.out_pred) a.out_pred[t[i]] = pred;
          if (a.out_err) a.out_err[t[i]] = err[i];
          if (a.loss_partial) {
            if (stage_loss) {  // the logarithms wait for the trip's barrier below
              double* st = lstage + ((trip & 1) * RT + i * GPB + g) * 3;
              st[0] = pred;
              st[1] = yy[i];
              st[2] = pp[i];
            } else if (sb[i]) {
              loss_acc2 += logloss_term(yy[i], pp[i], pred, a.eps);
            } else {
              loss_acc += logloss_term(yy[i], pp[i], pred, a.eps);
            }
          }
          err_acc += err[i];
        }
      } else if (stage_loss && l == 0) {
        lstage[((trip & 1) * RT + i * GPB + g) * 3] = -1.0;  // no row here (a score is in [0, 1] or NaN)
      }
    }
    if (stage_loss) {
      // The two logarithms of a row's loss term are ~200 dependent f64 instructions; computed by
      // lane 0 of every lane group they ran once per row and WAVE (validation forward, 100 k
      // rows: 38 of 27 + us).  Staged, the trip's rows are spread over the workgroup's threads.
      __syncthreads();
      if (tid < RT) {
        const double* st = lstage + ((trip & 1) * RT + tid) * 3;
        if (!(st[0] < 0.0)) {  // (slot tid is row base + tid of the launch)
          const double term = logloss_term(st[1], st[2], st[0], a.eps);
          if (seg && base + tid >= a.n_rows_a)
            loss_acc2 += term;
          else
            loss_acc += term;
        }
      }
    }
    ++trip;

    int32_t touched[R];
    if (warm) {
#pragma unroll
      for (int i = 0; i < R; ++i)  // lane l touches the 16 bytes of its own entry
        touched[i] = *reinterpret_cast<const int32_t*>(a.ell + int64_t(nxt[i]) * a.ell_stride +
                                                      16 * l);
    }
    if (REC && (a.slot_mark || H > 0)) {
      // after the residual is known: marks of the sparse-class entries, and the hot
      // entries' err * x * [q, 1, x] into the workgroup's LDS sums.  A single round (rows
      // of at most LPR entries) still has its entries parked in LDS.
      // (fixed-order hot sums meet at workgroup barriers: every group then makes the rounds
      // of the plan's longest row, whatever its own rows need)
      const bool fix_hot = FIX && H > 0;
      const int rounds_len = fix_hot ? a.hot_rounds * LPR : maxlen;
      // (hot tile: the matrix core ignores the execution mask, so the lane groups of a wavefront
      // make the rounds of its longest row together; a group past its own rows has no live entry)
      for (int pb = 0; TILE ? __ballot(pb < rounds_len) != 0 : pb < rounds_len; pb += LPR) {
        Entry em[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          if (rounds_len > LPR) {  // (never in the padded form)
            em[i] = a.ent[len[i] > 0 ? p0[i] + min(pb + l, len[i] - 1) : 0];
            if (pb + l >= len[i]) em[i] = Entry{0, 0, 0.0};
            if (FIX) ebuf[i * LPR + l] = em[i];
          } else {
            em[i] = ebuf[i * LPR + l];
          }
        }
        if (a.slot_mark) {
#pragma unroll
          for (int i = 0; i < R; ++i) {
            if (pb + l < len[i] && em[i].slot >= 0) {
              // the row's batch position and residual at the entry's slot (no atomic: the
              // row ids of a step are distinct), and the slot's bit in the map the gradient
              // launch scans (no-return atomic).  The mark is written through like the Q row,
              // as the two words {t, 0} and the residual; the fixed-order forms keep the plain
              // store (the other costs them two VGPRs, or 8 bytes of scratch at k = 32)
              if (!DET) {
                Pack<2> pm;
                pm.v[0] = __hiloint2double(0, int32_t(t[i]));
                pm.v[1] = err[i];
                pm.store_through(reinterpret_cast<double*>(a.slot_mark + em[i].slot));
              } else {
                a.slot_mark[em[i].slot] = SlotMark{int32_t(t[i]), 0, err[i]};
              }
              atomicOr(a.slot_bits + (em[i].slot >> 6), 1ull << (em[i].slot & 63));
            }
          }
        }
        if (!(H > 0)) continue;
        if constexpr (FIX) {
          // ---- park: Q rows (once), err * x * [1, x] in place of the entries, row sets ----
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const int row = i * GPB + g;
            if (pb == 0 && fok[0]) {
              Pack<VEC> pq;
#pragma unroll
              for (int v = 0; v < VEC; ++v) pq.v[v] = q[i][0][v];
              pq.store(Qs + row * KS + fo[0]);
            }
            const bool live = pb + l < len[i];
            if (live && em[i].slot < 0) {
              const int h = -1 - em[i].slot;
              atomicOr(&hbits[h * NW + (row >> 5)], 1u << (row & 31));
              hpos[h * PS + row] = uint8_t(l);
            }
            const double coef = live ? err[i] * em[i].x : 0.0;
            Pack<2> pc;
            pc.v[0] = coef;
            pc.v[1] = coef * em[i].x;
            pc.store(reinterpret_cast<double*>(ebuf + i * LPR + l));
          }
          __syncthreads();
          const Entry* ebase = reinterpret_cast<const Entry*>(dyn_lds + BLOCK);
          // sum of err * x * [q, 1, x] over the rows of a set (lo: rows base.., hi: rows
          // base + 64..), ascending; U rows' LDS reads are in flight together
          double acc[VEC], accw, accx;
          const auto add_rows = [&](int h, unsigned long long lo, unsigned long long hi, int base) {
            while (lo | hi) {
              constexpr int U = kHotUnroll;
              int rowu[U];
              bool ok[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                ok[u] = (lo | hi) != 0;
                int bit = 0;
                if (lo) {
                  bit = __builtin_ctzll(lo);
                  lo &= lo - 1;
                } else if (hi) {
                  bit = 64 + __builtin_ctzll(hi);
                  hi &= hi - 1;
                }
                rowu[u] = base + bit;
              }
              int ju[U];
#pragma unroll
              for (int u = 0; u < U; ++u) ju[u] = hpos[h * PS + rowu[u]] & (LPR - 1);
              Pack<2> cf[U];
              Pack<VEC> qv[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int gg = rowu[u] % GPB, ii = rowu[u] / GPB;
                cf[u].load(reinterpret_cast<const double*>(ebase + gg * (R * LPR + 1) + ii * LPR + ju[u]));
                qv[u].load(Qs + rowu[u] * KS + fo[0]);
              }
#pragma unroll
              for (int u = 0; u < U; ++u) {
                if (ok[u]) {
#pragma unroll
                  for (int v = 0; v < VEC; ++v) acc[v] += cf[u].v[0] * qv[u].v[v];
                  accw += cf[u].v[0];
                  accx += cf[u].v[1];
                }
              }
            }
          };
          const auto clear_acc = [&] {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
            accw = 0.0;
            accx = 0.0;
          };
          const auto add_to = [&](double* row_out, bool overwrite) {
            if (fok[0]) {
#pragma unroll
              for (int v = 0; v < VEC; ++v)
                row_out[fo[0] + v] = overwrite ? acc[v] : row_out[fo[0] + v] + acc[v];
            }
            if (l == 0) {
              row_out[k] = overwrite ? accw : row_out[k] + accw;
              row_out[k + 1] = overwrite ? accx : row_out[k + 1] + accx;
            }
          };
          // the NHV most frequent columns are cut into cells of 32 rows, one per lane group:
          // a cell's sum goes to its own row of `part`, combined in cell order below
          if (NCELL > 1 && g / NCELL < H) {
            const int h = g / NCELL, cell = g % NCELL;
            const unsigned int word = hbits[h * NW + cell];
            if (l == 0) hbits[h * NW + cell] = 0u;  // (the group has read it: one wave)
            clear_acc();
            add_rows(h, word, 0ull, cell * 32);
            add_to(part + g * hot_w, true);
          }
          // the other columns: one lane group each, dealt boustrophedon over the ranks (which
          // descend by frequency), starting opposite to the cells' order
          for (int s2 = 0; NHV + s2 * GPB < H; ++s2) {
            const int h = NHV + s2 * GPB + ((s2 & 1) ? g : GPB - 1 - g);
            if (h >= H) continue;
            unsigned long long lo = 0, hi = 0;
#pragma unroll
            for (int wi = 0; wi < NW; ++wi) {
              const unsigned long long word = hbits[h * NW + wi];
              if (wi < 2)
                lo |= word << (32 * wi);
              else
                hi |= word << (32 * (wi - 2));
            }
            if ((lo | hi) == 0) continue;
            if (l < NW) hbits[h * NW + l] = 0u;
            clear_acc();
            add_rows(h, lo, hi, 0);
            add_to(hot + h * hot_w, false);
          }
          __syncthreads();  // the next round / trip rewrites the entries
          if (NCELL > 1) {
            // cells of a column, in cell order (lane group h: nobody else touches hot[h])
            if (g < NHV && g < H) {
              double* hrow = hot + g * hot_w;
              for (int f = l; f < hot_w; f += LPR) {
                double sum = hrow[f];
#pragma unroll
                for (int c = 0; c < NCELL; ++c) sum += part[(g * NCELL + c) * hot_w + f];
                hrow[f] = sum;
              }
            }
          }
          continue;
        }
        if constexpr (TILE) {
          // ---- arrival-order hot sums, the most frequent columns on the matrix core ----
          // A live hot entry of rank h < kTileRanks is a TILE entry: its err * x * q goes into
          // G[rank][factor] += C[rank][row] * Q[row][factor], one v_mfma_f64_16x16x4 per row in
          // flight, tile of 16 ranks and factor parity -- the wavefront's four lane groups are
          // the four k-slots, lane j of a group holds factors 2j, 2j + 1 (the B operand as it
          // stands) -- and the tile is flushed into the LDS sums once per round.  The other
          // live hot entries are walked as before, compacted to the front of the round.
          constexpr int GPW = kWave / LPR;  // lane groups of a wave
          constexpr int NT = kTileRanks / 16;
          typedef double tile_acc __attribute__((ext_vector_type(4)));
          // (the lane's constants of this pass are derived here, from a value the compiler cannot
          // see through: hoisted out of the trip loop they would hold registers under the gathers)
          int tid_here = tid;
          asm volatile("" : "+v"(tid_here));
          const int lh = tid_here % LPR, gh = tid_here / LPR, gw = gh % GPW;
          HotEnt* const hbuf = reinterpret_cast<HotEnt*>(ebuf);
          double* const strip = hot + H * hot_w;  // [R][GPB][kTileRanks], behind the hot sums
          bool rowok[R], won[R];
          unsigned long long walked[R];  // the wave's lanes whose entry of row i is walked
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const bool live = pb + l < len[i] && em[i].slot < 0;
            const int h = -1 - em[i].slot;
            // Containment: a non-finite row of V reaches only the columns of the rows that hold
            // it, and 0 * NaN inside the tile would spread it.  A row that is not valid, or whose
            // residual is not finite, gives zeros to B and keeps all its hot entries on the walk.
            // A finite residual implies a finite q: any non-finite q[f] makes `pair` NaN.
            rowok[i] = valid[i] && __builtin_isfinite(err[i]);
            const bool tile_e = live && rowok[i] && h < kTileRanks;
            won[i] = live && !tile_e;
            walked[i] = __ballot(won[i]);
            const double coef = err[i] * em[i].x;
            if (live) {  // the [k] / [k+1] sums by the entry's own lane, tile entry or not
              double* const hsum = hot + (-em[i].slot * hot_w - 2);
              unsafeAtomicAdd(hsum, coef);
              unsafeAtomicAdd(hsum + 1, coef * em[i].x);
            }
            // A operand: lane r of the group gets the coefficient of the row's entry of rank r
            // (+ 16 per tile), 0 where the row has none -- through the group's strip (same
            // wavefront, program order; read back where the products are issued)
            double* const st = strip + (i * GPB + gh) * kTileRanks;
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) st[tl * 16 + lh] = 0.0;
            if (tile_e) st[h] = coef;
          }
          // the entries the wave walks: the largest count of a row of its groups (scalar)
          int wcnt = 0;
#pragma unroll
          for (int i = 0; i < R; ++i)
#pragma unroll
            for (int gq = 0; gq < GPW; ++gq)
              wcnt = max(wcnt, __popc(unsigned(walked[i] >> (gq * LPR)) & ((1u << LPR) - 1u)));
          // (the lane groups of a wave start at different entries, as adds to one LDS address
          // from several groups in one instruction serialise)
          const int rot = (gw * wcnt) / GPW;
#pragma unroll
          for (int i = 0; i < R; ++i) {
            // walked entries first, in lane order (an entry's place: the walked entries of its
            // row in lower lanes); the other lanes fill the positions behind them
            const unsigned bits = unsigned(walked[i] >> (gw * LPR)) & ((1u << LPR) - 1u);
            const int below = __popc(bits & ((1u << lh) - 1u));
            const int p = won[i] ? below : __popc(bits) + lh - below;
            const int at = p - rot < 0 ? p - rot + wcnt : p - rot;
            if (p < wcnt)
              hbuf[i * LPR + at] = HotEnt{won[i] ? (-1 - em[i].slot) * hot_w : -1, 0, err[i] * em[i].x};
          }
          // one factor parity at a time (the tile's registers are the pass's widest item)
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            tile_acc D[NT];
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) D[tl] = tile_acc{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < R; ++i) {
              const double* const st = strip + (i * GPB + gh) * kTileRanks;
              const double b = rowok[i] ? q[i][0][v] : 0.0;
#pragma unroll
              for (int tl = 0; tl < NT; ++tl)
                D[tl] = __builtin_amdgcn_mfma_f64_16x16x4f64(st[tl * 16 + lh], b, D[tl], 0, 0, 0);
            }
            // flush: D register `reg` of a lane is rank (lane >> 4) + 4 reg, factor 2 (lane & 15) + v
#pragma unroll
            for (int tl = 0; tl < NT; ++tl)
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int rank = tl * 16 + gw + 4 * reg;
                if (rank < H && fok[0]) unsafeAtomicAdd(hot + rank * hot_w + fo[0] + v, D[tl][reg]);
              }
          }
          for (int j = 0; j < wcnt; ++j) {
            HotEnt eh[R];
#pragma unroll
            for (int i = 0; i < R; ++i) eh[i] = hbuf[i * LPR + j];  // broadcast in the group
            // two rows of the group holding the same hot column: one add for both
            const bool pair01 = R == 2 && eh[0].off >= 0 && eh[0].off == eh[R - 1].off;
            const double coef2 = pair01 ? eh[R - 1].coef : 0.0;
            if (pair01) eh[R - 1].off = -1;
#pragma unroll
            for (int i = 0; i < R; ++i) {
              if (eh[i].off >= 0 && fok[0]) {
                double* hrow = hot + eh[i].off + fo[0];
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                  unsafeAtomicAdd(hrow + v, R == 2 && i == 0
                                                ? eh[0].coef * q[0][0][v] + coef2 * q[R - 1][0][v]
                                                : eh[i].coef * q[i][0][v]);
              }
            }
          }
          continue;
        }
        // ---- arrival-order hot sums (LDS float atomics) ----
        const int cnt = (maxlen - pb) < LPR ? (maxlen - pb) : LPR;
        // the entries of the round the wave walks: the largest count of its active groups
        // (one ballot per bit: the lanes of groups that have left the rounds take no part),
        // so that the walk below is a scalar loop
        int wcnt = 0;
#pragma unroll
        for (int b = LPR; b > 0; b >>= 1)
          if (__ballot(cnt >= (wcnt | b))) wcnt |= b;
        // the lane groups of a wave start at different entries: rows of one log
        // tend to hold the same hot column at the same position, and adds to one
        // LDS address from several groups in one instruction serialise
        const int rot = ((g % (kWave / LPR)) * wcnt) / (kWave / LPR);
        // each lane prepares its own entry once: the offset of its column's sums in `hot`
        // (-1: not a hot entry, or past the row's end) and err * x, written over the round's
        // records at position l - rot of the walk; and it adds the entry's [k] / [k+1] sums
        // itself (the lanes of a row hold distinct columns)
        HotEnt* const hbuf = reinterpret_cast<HotEnt*>(ebuf);
        const int at = l - rot < 0 ? l - rot + wcnt : l - rot;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const bool on = pb + l < len[i] && em[i].slot < 0;
          const int off = on ? (-1 - em[i].slot) * hot_w : -1;
          const double coef = err[i] * em[i].x;
          if (l < wcnt) hbuf[i * LPR + at] = HotEnt{off, 0, coef};
          if (on) {  // (-slot * hot_w - 2 = off + k: no k in a scalar register here)
            double* const hsum = hot + (-em[i].slot * hot_w - 2);
            unsafeAtomicAdd(hsum, coef);
            unsafeAtomicAdd(hsum + 1, coef * em[i].x);
          }
        }
        for (int j = 0; j < wcnt; ++j) {
          HotEnt eh[R];
#pragma unroll
          for (int i = 0; i < R; ++i) eh[i] = hbuf[i * LPR + j];  // broadcast in the group
          // two rows of the group holding the same hot column: one add for both
          const bool pair01 = R == 2 && eh[0].off >= 0 && eh[0].off == eh[R - 1].off;
          const double coef2 = pair01 ? eh[R - 1].coef : 0.0;
          if (pair01) eh[R - 1].off = -1;
#pragma unroll
          for (int i = 0; i < R; ++i) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              if (eh[i].off >= 0 && fok[c]) {
                double* hrow = hot + eh[i].off + fo[c];
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                  unsafeAtomicAdd(hrow + v, R == 2 && i == 0
                                                ? eh[0].coef * q[0][c][v] + coef2 * q[R - 1][c][v]
                                                : eh[i].coef * q[i][c][v]);
              }
            }
          }
        }
      }
    }
    if (warm) {
#pragma unroll
      for (int i = 0; i < R; ++i) asm volatile("" ::"v"(touched[i]));  // keep the touches alive
    }
  }

  if (H > 0) {
    __syncthreads();
    // slab layout [H][gridDim.x][k+2]: the slabs of one column are contiguous.  An even k makes
    // a row of k + 2 doubles whole 16-byte pairs, here and in LDS: one write-through store each
    // (the gradient launch reads the slabs next)
    if constexpr (REC && VEC == 2) {
      for (int i = 2 * tid; i < H * hot_w; i += 2 * BLOCK) {
        const int h = i / hot_w, f = i % hot_w;
        Pack<2> ps;
        ps.load(hot + i);
        ps.store_through(a.hot_slab + (int64_t(h) * gx + bx) * hot_w + f);
      }
    } else {
      for (int i = tid; i < H * hot_w; i += BLOCK) {
        const int h = i / hot_w, f = i % hot_w;
        a.hot_slab[(int64_t(h) * gx + bx) * hot_w + f] = hot[i];
      }
    }
  }
  if (a.err_partial) {
    const double s = block_sum<BLOCK>(err_acc, red);
    if (tid == 0) a.err_partial[bx] = s;
  }
  if (a.loss_partial) {
    const double s = block_sum<BLOCK>(loss_acc, red);
    if (tid == 0) a.loss_partial[bx] = s;
  }
  if (seg && a.loss_partial2) {
    const double s = block_sum<BLOCK>(loss_acc2, red);
    if (tid == 0) a.loss_partial2[bx] = s;
  }
}

// loss = -(sum of partials)/n, fixed order
__global__ __launch_bounds__(kBlock) void loss_finish_kernel(const double* partial, int n_partial,
                                                            int64_t n_rows, double* out) {
  __shared__ double lds[kBlock];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
  const double s = block_sum<kBlock>(acc, lds);
  if (threadIdx.x == 0) out[0] = -s / double(n_rows);
}

// the same for a run of launches at once: block b finishes the partials of launch b
__global__ __launch_bounds__(kBlock) void loss_finish_many_kernel(const double* partial,
                                                                 int64_t stride, int n_partial,
                                                                 int64_t n_rows, double* out) {
  __shared__ double lds[kBlock];
  const double* row = partial + int64_t(blockIdx.x) * stride;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += row[i];
  const double s = block_sum<kBlock>(acc, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = -s / double(n_rows);
}

// standalone IPS log-loss of given scores (src/base.py:37-61)
__global__ __launch_bounds__(kBlock) void logloss_kernel(const double* y, const double* pred,
                                                        const double* pscore,
                                                        const int32_t* row_ids, int64_t n_rows,
                                                        double eps, double* partial) {
  __shared__ double lds[kBlock];
  double acc = 0.0;
  for (int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x; t < n_rows;
       t += int64_t(gridDim.x) * kBlock) {
    const int64_t r = row_ids ? int64_t(row_ids[t]) : t;
    acc += logloss_term(y[r], pscore[r], pred[t], eps);
  }
  const double s = block_sum<kBlock>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------
// fixed-order reductions over rows of a table (used by launches 2 and 3)
// ---------------------------------------------------------------------------
// tot[f] = sum over the valid rows r < rows of row(r)[f], f < width, in a fixed order: the
// block's threads split into row groups x factor lanes, each group sums its rows in ascending
// order (U loads in flight per thread), the groups are then added in group order.
// Rows: row(r) = where row r starts, valid(row) = whether it counts.
template <int U, class Rows>
__device__ inline void ordered_rows_sum(const Rows& from, int rows, int width,
                                        double* scratch /*[kBlock]*/, double* tot /*[width]*/) {
  const int fw = width < kBlock ? width : kBlock;  // factor lanes per row group
  const int nsg = kBlock / fw;
  const int sg = threadIdx.x / fw, fl = threadIdx.x % fw;
  const bool live = sg < nsg;
  for (int f0 = 0; f0 < width; f0 += fw) {
    const int f = f0 + fl;
    double acc = 0.0;
    if (live && f < width) {
      for (int r = sg; r < rows; r += nsg * U) {
        const double* row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = from.row(r + u * nsg < rows ? r + u * nsg : r);
        double v[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          v[u] = row[u][f];
          const bool counts = from.valid(row[u]);  // (read whether or not the row is in range)
          ok[u] = counts && r + u * nsg < rows;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += ok[u] ? v[u] : 0.0;
      }
    }
    __syncthreads();
    scratch[threadIdx.x] = acc;
    __syncthreads();
    if (sg == 0 && f < width) {
      double s = 0.0;
      for (int j = 0; j < nsg; ++j) s += scratch[j * fw + fl];
      tot[f] = s;
    }
  }
  __syncthreads();
}

// the forward workgroups' slabs of one hot column: contiguous rows of `width`, all of them valid
// (32 loads in flight: one round covers the slabs of a small batch's forward -- 125 workgroups at
// B = 2 000 -- with seven row groups at k = 32)
struct SlabRows {
  const double* base;
  int width;
  __device__ const double* row(int r) const { return base + int64_t(r) * width; }
  __device__ bool valid(const double*) const { return true; }
};

// the partial rows first .. of one split column ([k+3] each), valid iff stamped with this step
struct PartRows {
  const double* parts;
  int first, k;
  double stamp;
  __device__ const double* row(int r) const { return parts + int64_t(first + r) * (k + 3); }
  __device__ bool valid(const double* row) const { return row[k + 2] == stamp; }
};

// ---------------------------------------------------------------------------
// 2. sparse-class gradient + update (tasks of whole columns), hot columns, w0
// ---------------------------------------------------------------------------
struct WinRec {  // a marked slot of the word being processed, parked in LDS, 24 B
  int32_t t;     // batch position of the slot's row
  int32_t col;   // feature column
  double coef;   // err_t * x
  double cx;     // err_t * x * x
};

// what launches 2 and 3 both need to finish a column
struct ColArgs {
  double* V;        // apply mode: updated in place; grad mode: read only
  double* w;
  int32_t k;
  int64_t n;        // features
  double lr;
  double* grad;     // nullable: grad mode -> [G_V | g_w | g_w0]
  int32_t* touch;   // nullable (grad mode): touch[col] = touch_id for every column written
  int32_t touch_id;
  double* parts;    // [n_parts][k+3]: M[0..k), sum coef, sum coef*x, step stamp (split columns)
  double stamp;     // id of this step (a partial row is valid iff its stamp matches)
};

struct ConsArgs {
  ColArgs c;
  const TaskRec* tasks;  // [nb_tasks * tasks per workgroup]
  int32_t task_words;    // 64-slot words of the slot bitmap per task
  int32_t pool;          // single-chunk forms: deal a workgroup's marks evenly (consume_pools)
  unsigned long long* slot_bits;  // one bit per slot: set by the forward, cleared here
  unsigned long long* slot_bits_other;  // CH form: the bitmap of the step before, cleared here
  const SlotMark* slot_mark;      // {batch position, residual} of a marked slot's row
  const SlotRec* slots;
  const double* Q;
  double* w0;
  // the hot columns and w0 ride in the same launch: the workgroups after the tasks reduce
  // the forward's slabs / residual sums (independent of the sparse class, so they overlap)
  int32_t nb_tasks;  // workgroups that process tasks
  int32_t n_hot;
  const int32_t* hot_cols;
  const double* hot_slab;
  int32_t n_slabs;
  const double* err_partial;  // [n_slabs] per-workgroup sums of the residual
  int32_t n_chunks;           // CH form: chunks of 64 lanes x VEC factors (fm_chunks)
  int32_t xcd_chunks;         // CH form: 1 = chunks dealt to XCDs (1-D grid), 0 = blockIdx.y
};

// Whether the gradient launch of a plan deals a workgroup's marks evenly to its groups: where a
// task expects more marks per max_batch step than one batch of the chain (kConsBatch entries).
// A plan cuts its tasks for kTaskMarks = 8 expected marks; it stays below that only where
// task_words is capped by the lanes of a group -- small batches, 2 marks at B = 2 000 of 10^6 rows.
constexpr int kConsBatch = 4;
inline bool consume_pools(int task_words, int64_t max_batch, int64_t n_rows) {
  return int64_t(task_words) * 64 * max_batch > int64_t(kConsBatch) * n_rows;
}

// chunks of 64 lanes x vec factors that cover a row of k factors
inline int fm_chunks(int k, int vec) { return ((k + vec - 1) / vec + 63) / 64; }

// The sums of one column in a lane group: the lane's VEC factors of M (factor f = first factor of
// the group's chunk + lane * VEC on), sum coef, sum coef * x.  A [k+3] row -- a group's head row
// in LDS, a partial row in memory -- holds the same: [0..k) M, [k] sum coef, [k+1] sum coef * x;
// its word [k+2] belongs to the caller (flags of a head row, the stamp of a partial row).
template <int VEC>
struct ColAcc {
  double m[VEC];
  double gw, d;
  __device__ inline void clear() {
#pragma unroll
    for (int v = 0; v < VEC; ++v) m[v] = 0.0;
    gw = 0.0;
    d = 0.0;
  }
  // into a row; the scalar part by the one lane that has `scalars`
  __device__ inline void store_row(double* row, int f, int k, bool scalars) const {
    if (f < k) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) row[f + v] = m[v];
    }
    if (scalars) {
      row[k] = gw;
      row[k + 1] = d;
    }
  }
  // += a row
  __device__ inline void add_row(const double* row, int f, int k) {
    if (f < k) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) m[v] += row[f + v];
    }
    gw += row[k];
    d += row[k + 1];
  }
  // a row read whole before it is known whether it counts (fc = f, or 0 past the row's end), ...
  __device__ inline void load_row(const double* row, int fc, int k) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) m[v] = row[fc + v];
    gw = row[k];
    d = row[k + 1];
  }
  // ... then added if it does
  __device__ inline void add_if(bool ok, const ColAcc& o) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) m[v] += ok ? o.m[v] : 0.0;
    gw += ok ? o.gw : 0.0;
    d += ok ? o.d : 0.0;
  }
};

// the lane's factors of V[col,:] (any factors of the row where the lane has none: f >= k)
template <int VEC>
__device__ inline Pack<VEC> load_v_row(const double* V, int32_t col, int k, int f) {
  Pack<VEC> p;
  p.load(V + int64_t(col) * k + (f < k ? f : 0));
  return p;
}

// THE UPDATE RULE.  A factor of V from the sums of its column (m = sum coef * Q[t,f], d = sum
// coef * x; vold = the factor as it was read before): its gradient g = d * vold - m, or its new
// value vold - lr * g.  The roundings are spelled out, because the results are compared bit for
// bit from build to build: the step is one fused multiply-add; so is g, except where `dv_rounded`
// asks for the product d * vold rounded on its own before the subtraction.  That is the first
// factor of a lane at the lane-group sites (apply_column), and a record of how the expression
// came out of the compiler when every site spelled it for itself -- the product both branches
// share was hoisted for the first factor only.  One rounding everywhere would be the better rule
// and a change of results.
__device__ inline double updated_factor(double vold, double m, double d, double lr, bool grad,
                                        bool dv_rounded) {
  double g;
  if (dv_rounded) {
#pragma clang fp contract(off)
    const double dv = d * vold;
    g = dv - m;
  } else {
    g = fma(d, vold, -m);
  }
  return grad ? g : fma(lr, -g, vold);
}

// THE OPTIMISER of the update sites (apply_scalar, apply_column, apply_column_block and the long
// columns of fm_finalize_chunk_kernel), a type parameter of launches 2 and 3.  SgdRule
// (rfm_rule.hpp): theta -= lr * g as spelled above, the form every site had before there was a
// choice; its instantiations take the branches they always took.  AdaGradRule: every element of
// w0, w and V has an accumulator G of its own and takes adagrad_element's step, with g the
// element's gradient exactly as gradient mode writes it (so -s for a scalar, updated_factor(...,
// grad = true, ...) for a factor).  g = 0 changes neither, so a hot column without an entry in the batch
// keeps its bits although it is visited; an untouched column of the sparse class is not visited.
// Gradient mode never runs under AdaGradRule (enqueue_step).
struct AdaGradRule {
  static constexpr bool kAda = true;
  double* acc_V;   // [n][k]
  double* acc_w;   // [n]
  double* acc_w0;  // [1]
  double eps;
};

// *p += x by its only writer of the step.  As `*p += x` the wavefront stands still for the load of *p
// (nothing else waits for it) -- once per finished column in the gradient launch, eight times per task
// where columns are short, and one dependent level in the finalize; the no-return atomic add gives the
// same sum without the wait.
__device__ inline void add_by_only_writer(double* p, double x) { unsafeAtomicAdd(p, x); }

// ... and a scalar parameter from the sum s of its residual terms, by one thread: *p += lr * s in
// place, or grad[n*k + at] = -s.  (AdaGradRule, G = the element's accumulator: its step is no sum,
// so the element's only writer reads, computes and writes both.)
template <class O>
__device__ inline void apply_scalar(const ColArgs& c, const O& o, double* p, double* G, int64_t at,
                                    double s) {
  if constexpr (O::kAda) {
    double gacc = *G;
    *p = adagrad_element(*p, -s, c.lr, o.eps, &gacc);
    *G = gacc;
  } else {
    if (c.grad)
      c.grad[c.n * c.k + at] = -s;
    else
      add_by_only_writer(p, c.lr * s);
  }
}

// w[col] so, with the column's mark in touched-row mode (the row is valid for this step)
template <class O>
__device__ inline void apply_w(const ColArgs& c, const O& o, int32_t col, double gw) {
  if constexpr (O::kAda) {
    apply_scalar(c, o, c.w + col, o.acc_w + col, col, gw);
  } else {
    apply_scalar(c, o, c.w + col, nullptr, col, gw);
    if (c.grad && c.touch) c.touch[col] = c.touch_id;
  }
}

// the lane's factors of a column's accumulator row, requested where its row of V is
template <int VEC, class O>
__device__ inline void load_acc_row(const O& o, Pack<VEC>& p, int32_t col, int k, int f) {
  if constexpr (O::kAda) p.load(o.acc_V + int64_t(col) * k + (f < k ? f : 0));
}

// V[col,:] and w[col] from the sums of one column in a lane group: update in place, or write the
// gradient row (grad mode).  vold = the lane's factors f.. of the row as they were read before
// (gold: of its accumulator row, AdaGradRule only);
// `scalars`: this lane writes w / touch (lane 0 of the group that has the row's first chunk).
template <int VEC, class O>
__device__ inline void apply_column(const ColArgs& c, const O& o, int32_t col, const ColAcc<VEC>& acc,
                                    const Pack<VEC>& vold, const Pack<VEC>& gold, int f, bool scalars) {
  if constexpr (O::kAda) {
    if (f < c.k) {
      Pack<VEC> out, gout;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        gout.v[v] = gold.v[v];
        const double g = updated_factor(vold.v[v], acc.m[v], acc.d, c.lr, true, v == 0);
        out.v[v] = adagrad_element(vold.v[v], g, c.lr, o.eps, &gout.v[v]);
      }
      out.store(c.V + int64_t(col) * c.k + f);
      gout.store(o.acc_V + int64_t(col) * c.k + f);
    }
    if (scalars) apply_w(c, o, col, acc.gw);
  } else {
    if (f < c.k) {
      Pack<VEC> out;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        out.v[v] = updated_factor(vold.v[v], acc.m[v], acc.d, c.lr, c.grad != nullptr, v == 0);
      out.store((c.grad ? c.grad : c.V) + int64_t(col) * c.k + f);
    }
    if (scalars) apply_w(c, o, col, acc.gw);
  }
}

// The same from a whole workgroup, sums in LDS: tot[0..k) = M, tot[k] = sum coef,
// tot[k+1] = sum coef*x.
// (vpre: the row as the caller read it before the sums were formed -- threadIdx.x + j * kBlock
// -- so that the load is in flight beside the sums' own loads; null: read here.  gpre: the
// accumulator row so, with vpre)
constexpr int kRowPre = (RFM_MAX_FACTORS + kBlock - 1) / kBlock;
template <class O>
__device__ inline void apply_column_block(const ColArgs& c, const O& o, int32_t col, const double* tot,
                                          const double* vpre = nullptr, const double* gpre = nullptr) {
  const int k = c.k;
  const double gw = tot[k], d = tot[k + 1];
  int j = 0;
  for (int f = threadIdx.x; f < k; f += kBlock, ++j) {
    const int64_t at = int64_t(col) * k + f;
    const double vold = vpre ? vpre[j] : c.V[at];
    if constexpr (O::kAda) {
      double gacc = vpre ? gpre[j] : o.acc_V[at];
      const double g = updated_factor(vold, tot[f], d, c.lr, true, false);
      c.V[at] = adagrad_element(vold, g, c.lr, o.eps, &gacc);
      o.acc_V[at] = gacc;
    } else {
      (c.grad ? c.grad : c.V)[at] = updated_factor(vold, tot[f], d, c.lr, c.grad != nullptr, false);
    }
  }
  if (threadIdx.x == 0) apply_w(c, o, col, gw);
}

// slots a lane group handles per pass over a 64-slot word of the bitmap: PLANES pieces of
// LPR consecutive slots
template <int LPR>
struct WinShape {
  static constexpr int PLANES = LPR >= 64 ? 1 : (LPR == 32 ? 2 : 4);
  static constexpr int WIN = PLANES * LPR;  // 64 for LPR >= 16; 16 / 32 for LPR = 4 / 8
  // LDS of a lane group: the parked records and the list of the slots it has marked
  static constexpr int kGroupBytes = WIN * (int(sizeof(WinRec)) + 8);
};

// LDS of a workgroup of fm_consume_kernel: per group the list of marked slots and their parked
// records, then the groups' head rows, then how many slots each group listed (one int each); or
// (hot-column / w0 workgroups) reduction scratch and totals
constexpr int kConsHotBytes = (kBlock + 1024 + 2) * int(sizeof(double));
template <int LPR>
constexpr size_t consume_lds_bytes_of(int k) {
  constexpr size_t gpb = kBlock / LPR;
  const size_t tasks = gpb * WinShape<LPR>::kGroupBytes + gpb * size_t(k + 3) * sizeof(double) +
                       (gpb * sizeof(int32_t) + 7) / 8 * 8;
  return tasks > size_t(kConsHotBytes) ? tasks : size_t(kConsHotBytes);
}
inline size_t consume_lds_bytes(int lpr, int k) {
  switch (lpr) {
    case 4: return consume_lds_bytes_of<4>(k);
    case 8: return consume_lds_bytes_of<8>(k);
    case 16: return consume_lds_bytes_of<16>(k);
    case 32: return consume_lds_bytes_of<32>(k);
    default: return consume_lds_bytes_of<64>(k);
  }
}

// inclusive prefix sum over the LPR lanes of a lane group
template <int LPR>
__device__ inline int group_scan(int v, int l) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) {
    const int up = __shfl_up(v, o, LPR);
    if (l >= o) v += up;
  }
  return v;
}

// A hot column, by one workgroup: the forward workgroups' slabs, in block order; the column's row
// of V is requested first, so that it arrives with the slabs and not after them.
template <class O>
__device__ inline void consume_hot_column(const ConsArgs& a, const O& o, int hb, double* lds) {
  const int k = a.c.k;
  const int32_t col = a.hot_cols[hb];
  double vpre[kRowPre];
#pragma unroll
  for (int j = 0; j < kRowPre; ++j) {
    const int f = int(threadIdx.x) + j * kBlock;
    vpre[j] = a.c.V[int64_t(col) * k + (f < k ? f : 0)];
  }
  double gpre[kRowPre];
  if constexpr (O::kAda) {
#pragma unroll
    for (int j = 0; j < kRowPre; ++j) {
      const int f = int(threadIdx.x) + j * kBlock;
      gpre[j] = o.acc_V[int64_t(col) * k + (f < k ? f : 0)];
    }
  }
  double* tot = lds + kBlock;
  ordered_rows_sum<32>(SlabRows{a.hot_slab + int64_t(hb) * a.n_slabs * (k + 2), k + 2}, a.n_slabs,
                       k + 2, lds, tot);
  if constexpr (O::kAda)
    apply_column_block(a.c, o, col, tot, vpre, gpre);
  else
    apply_column_block(a.c, o, col, tot, vpre);
}

// w0, by one workgroup, from the forward workgroups' residual sums
template <class O>
__device__ inline void consume_w0(const ConsArgs& a, const O& o, double* lds) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.n_slabs; i += kBlock) acc += a.err_partial[i];
  const double s = block_sum<kBlock>(acc, lds);
  if (threadIdx.x == 0) {
    if constexpr (O::kAda)
      apply_scalar(a.c, o, a.w0, o.acc_w0, a.c.n, s);
    else
      apply_scalar(a.c, o, a.w0, nullptr, a.c.n, s);
  }
}

// One TASK per lane group: `task_words` 64-slot words of the slot view, the same number for
// every task of a plan (chosen so that a task expects a handful of marked slots), so the
// task's bitmap words are the kernel's FIRST load -- nothing has to be looked up before
// them.  Whole columns are packed into the tasks in column order; a column may run over
// several consecutive tasks, but never over the edge of a workgroup's tasks unless it is
// longer than all of them together.  The group lists the task's marked slots, in slot
// order, in LDS, then runs the chain ONCE: the marked slots' records and marks (parked in
// LDS) -> Q rows and V rows (eight gathers in flight) -> err*x*[Q[t,:], 1, x] accumulated
// strictly in slot order.  A column that lies inside the task is updated in place -- this
// group is its only writer.  For a column that continues from the previous task the sums
// go to LDS (`head` row of the group); the group in whose task such a column STARTS owns
// it: after a workgroup barrier it adds the followers' head rows in task (= slot) order to
// its own and updates the column.  Only a column longer than a whole workgroup's tasks
// leaves partial rows in memory (one per workgroup) for fm_finalize_kernel.  The work of a
// launch follows the batch (marked slots): an untouched task reads its bitmap words and
// waits at the barrier.  (Single-chunk forms, plans whose tasks expect more than one batch of
// the chain: the chain runs over an even share of the workgroup's listed slots instead of the
// group's own list -- see "dealt evenly" in the kernel.)
// (The lane groups of a wave run in lock step: ballots and shuffles are wave-wide.)
// A lane holds VEC factors of a row: one chunk of LPR x VEC factors covers it, or -- CH, factor
// counts of more than one chunk per lane -- the chunks of a row are dealt to DIFFERENT workgroups
// (blockIdx.y = chunk), so that a task's chain is one 16-byte load per lane and entry whatever
// the chunk count, and that many times as many lane groups share the step's entries (measured at
// k = 400, B = 2 000: equal to a form with all chunks in registers within noise -- both wait on the
// same chain of dependent levels -- at half the registers and with one instantiation for every
// chunk count).  Every
// chunk lists the task's marks itself (same bitmap words: they hit in L2), so the words cannot be
// cleared while a sibling may still read them: the bitmap is double-buffered by step parity and
// chunk 0 clears the task's words of the OTHER buffer (the step before, long consumed).
constexpr int kConsChBatch = 4;  // CH form: entries whose Q and V rows are in flight together
// O: the update rule (SgdRule: the arguments are ConsArgs; AdaGradRule: ConsArgs with the rule behind).
template <int LPR, int VEC, bool CH = false, class O = SgdRule>
__global__ __launch_bounds__(kBlock, 1) void fm_consume_kernel(ArgsUnder<ConsArgs, O> a) {
  const O& o = rule_of(a);
  constexpr int GPB = kBlock / LPR;  // tasks of a workgroup
  constexpr int PLANES = WinShape<LPR>::PLANES;
  constexpr int WIN = WinShape<LPR>::WIN;  // marked slots a group lists before it runs the chain
  constexpr int BATCH = CH ? kConsChBatch : 4;  // entries whose Q and V rows are in flight together
  // CH: which chunk and which group of tasks this workgroup takes.  Workgroups go to the eight
  // XCDs round robin by their linear id, and every XCD has an L2 of its own: with the chunks
  // dealt to XCDs (chunk c = the XCDs [8c / n, 8(c+1) / n)) an XCD only ever touches ITS slice of
  // the Q rows and of V -- a quarter of them at k = 400 -- instead of all of both.
  int bx = int(blockIdx.x), chunk = 0;
  if (CH) {
    if (a.xcd_chunks) {
      const int xcd = bx & 7, slot = bx >> 3, nch = a.n_chunks;
      chunk = xcd * nch / 8;
      const int first = (chunk * 8 + nch - 1) / nch, next = ((chunk + 1) * 8 + nch - 1) / nch;
      bx = slot * (next - first) + (xcd - first);
      if (bx >= a.nb_tasks + a.n_hot + 1) return;  // (the grid is rounded up)
    } else {
      chunk = int(blockIdx.y);
    }
  }
  const int fb = chunk * (LPR * VEC);  // first factor of this workgroup's chunk
  constexpr int TRIPS = kTaskTrips;        // bitmap words a lane loads (task_words <= TRIPS*LPR)
  constexpr int kGroupBytes = WinShape<LPR>::kGroupBytes;
  extern __shared__ double lds_raw[];  // consume_lds_bytes(LPR, k)
  const ColArgs& c = a.c;
  const int k = c.k;
  // the hot-column workgroups and the one of w0 come last in the grid (measured: first, they
  // delay the tasks and the launch takes longer)
  if (bx >= a.nb_tasks) {
    if (CH && chunk != 0) return;
    const int hb = bx - a.nb_tasks;
    if (hb < a.n_hot)
      consume_hot_column(a, o, hb, lds_raw);
    else
      consume_w0(a, o, lds_raw);
    return;
  }
  const int lane = threadIdx.x % kWave;
  const int l = lane % LPR;
  const int gb = threadIdx.x / LPR;  // group in the workgroup
  const int f = fb + l * VEC;        // this lane's first factor
  const bool scalars = l == 0 && fb == 0;  // the lane that writes a column's scalar part to memory
  const int task = bx * GPB + gb;
  const int W = a.task_words;
  const int32_t slot0 = task * W * 64;  // first slot of the task
  // first loads: the task's bitmap words (one per lane and trip) and its description
  unsigned long long wd[TRIPS];
#pragma unroll
  for (int u = 0; u < TRIPS; ++u) {
    const int idx = u * LPR + l;
    wd[u] = idx < W ? a.slot_bits[int64_t(task) * W + idx] : 0ull;
  }
  const TaskRec tk = a.tasks[task];
#pragma unroll
  for (int u = 0; u < TRIPS; ++u) {
    if (CH) {
      if (fb == 0 && u * LPR + l < W) a.slot_bits_other[int64_t(task) * W + u * LPR + l] = 0ull;
    } else if (wd[u]) {
      a.slot_bits[int64_t(task) * W + u * LPR + l] = 0ull;  // consumed: cleared at once
    }
  }

  char* gmem = reinterpret_cast<char*>(lds_raw) + gb * kGroupBytes;
  WinRec* wrec = reinterpret_cast<WinRec*>(gmem);
  int32_t* list = reinterpret_cast<int32_t*>(gmem + WIN * sizeof(WinRec));
  double* heads = reinterpret_cast<double*>(reinterpret_cast<char*>(lds_raw) + GPB * kGroupBytes);
  double* head = heads + gb * (k + 3);  // the group's head row; [k+2] flags

  // the columns at the edges of what this group sums: of its task (from the plan), or of its part
  // of the workgroup's pooled marks (from the marks themselves, below)
  bool head_open = tk.flags & 1;  // first_col continues from the previous task / part
  bool tail_open = tk.flags & 2;  // last_col continues into the next task / part
  int32_t first_col = tk.first_col, last_col = tk.last_col;
  ColAcc<VEC> acc;
  acc.clear();
  Pack<VEC> vold;       // V row of the column being accumulated
  int32_t cur = -1;     // that column (uniform in the lane group)
  int fill = 0;         // marked slots listed and not yet consumed (uniform in the lane group)
  bool head_done = false;
  Pack<VEC> gold;       // AdaGradRule: the accumulator row of the column being accumulated (with vold)

  // a finished column: into the head row (continues from the previous task), or updated in
  // place; the last column of a tail-open task stays in `acc` for the combine below
  const auto finish = [&]() {
    if (head_open && cur == first_col) {
      acc.store_row(head, f, k, l == 0);
      head_done = true;
    } else {
      apply_column(c, o, cur, acc, vold, gold, f, scalars);
    }
  };

  // the chain over `fill` marked slots; slot_of(e) = the e-th of them (slot0 where e >= fill),
  // planes = an upper bound of every group's fill (uniform in the workgroup)
  const auto run_list = [&](auto slot_of, int planes) {
    // records and marks of the slots, parked in LDS by position
    SlotRec sr[PLANES];
    SlotMark mk[PLANES];
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) {
      if (pl * LPR < planes) {
        const int32_t s = slot_of(pl * LPR + l);
        mk[pl] = a.slot_mark[s];
        sr[pl] = a.slots[s];
      }
    }
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) {
      const int e = pl * LPR + l;
      if (pl * LPR < planes && e < fill) {
        const double coef = mk[pl].err * sr[pl].x;
        wrec[e] = WinRec{mk[pl].t, sr[pl].col, coef, coef * sr[pl].x};
      }
    }
    // every group of the wave loops as long as any of them has entries left
    int at = 0;
    while (__ballot(at < fill)) {
      const int nb = max(min(BATCH, fill - at), 0);
      WinRec rec[BATCH];
      Pack<VEC> qq[BATCH], vv[BATCH], ga[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        rec[u] = wrec[u < nb ? at + u : 0];
        if (u >= nb) {  // nothing there: any row of Q / V will do
          rec[u].t = 0;
          rec[u].col = 0;
        }
        // the entry's Q row, and the V row of its column in case the entry starts a new
        // column: fetched together, so that a run of one-entry columns (one-hot users and
        // items in a small batch) costs one round trip, not one per column
        qq[u].load(a.Q + int64_t(rec[u].t) * k + (f < k ? f : 0));
        // (an entry of the column the one before it belongs to needs no V row)
        if (rec[u].col != (u == 0 ? cur : rec[u > 0 ? u - 1 : 0].col)) {
          vv[u] = load_v_row<VEC>(c.V, rec[u].col, k, f);
          load_acc_row(o, ga[u], rec[u].col, k, f);
        }
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        if (u < nb) {
          if (rec[u].col != cur) {
            if (cur >= 0) finish();
            acc.clear();
            cur = rec[u].col;
            vold = vv[u];
            if constexpr (O::kAda) gold = ga[u];
          }
          const double coef = rec[u].coef, cx = rec[u].cx;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.m[v] += coef * qq[u].v[v];
          acc.gw += coef;
          acc.d += cx;
        }
      }
      at += nb;
    }
    fill = 0;
  };

  const auto own_slot = [&](int e) -> int32_t { return e < fill ? list[e] : slot0; };
  // ---- the workgroup's marks, dealt evenly to its groups ------------------------------------
  // What a task gets is a draw around what the plan expects, and the workgroup waits for its
  // longest chain.  So the chain does not run over a group's own list: every group lists its
  // task, the lists laid end to end are the workgroup's T marked slots in slot order, and group g
  // runs the chain over the positions [g * per, (g + 1) * per) of that pool, per = ceil(T / GPB)
  // -- its PART.  Which columns come into a part and go on behind it is read off the marks
  // (the columns of the positions before and behind the part), not off the plan.  A workgroup in
  // which a task has more marks than a list holds runs the tasks as they are instead.  So does
  // every workgroup of a plan whose tasks expect no more than one batch of the chain (a.pool = 0:
  // small batches, where a task's chain is one batch whatever it gets and the exchange below
  // would only stand in front of the first load).
  bool pooled = false;
  int32_t next_col = -2;  // pooled: column of the position behind the part (-2: there is none)
  if constexpr (!CH) if (a.pool) {
    bool over = false;  // the task has more marks than the list holds (uniform in the group)
#pragma unroll
    for (int u = 0; u < TRIPS; ++u) {
      // the task's marked slots into the list in lane (= slot) order, as far as the list has room
      unsigned long long word = wd[u];
      const int32_t s0 = slot0 + (u * LPR + l) * 64;
      const int cnt = __popcll(word);
      const int upto = group_scan<LPR>(cnt, l);
      const int take = min(cnt, max(WIN - fill - (upto - cnt), 0));
      int pos = fill + upto - cnt;
      for (int i = 0; i < take; ++i) {
        list[pos++] = s0 + (__ffsll((long long)word) - 1);
        word &= word - 1ull;
      }
      fill += __shfl(upto, LPR - 1, LPR);
      over |= fill > WIN;
    }
    int32_t* fills = reinterpret_cast<int32_t*>(heads + GPB * (k + 3));
    if (l == 0) fills[gb] = over ? WIN + 1 : fill;
    __syncthreads();
    // lane j < GPB of every wave: the fill of group j and the fills before it
    const int gl = lane % GPB;
    const int mine = fills[gl];
    const int incl = group_scan<GPB>(mine, gl);
    const int excl = incl - mine;
    if (__ballot(mine > WIN) == 0ull) {  // (the same in every wave of the workgroup)
      pooled = true;
      const int T = __builtin_amdgcn_readlane(incl, GPB - 1);
      const int per = (T + GPB - 1) / GPB;
      const int p0 = gb * per;
      const int n = max(min(per, T - p0), 0);  // empty parts come last
      // the slot at pooled position p (slot0 unless ok): the list it lies in is the last one
      // that starts at or before p, found by bisection of the prefix sums
      const auto pooled_slot = [&](int p, bool ok) -> int32_t {
        const int pc = max(min(p, T - 1), 0);
        int o = 0;
#pragma unroll
        for (int st = GPB / 2; st > 0; st >>= 1) o += __shfl(excl, o + st) <= pc ? st : 0;
        const int i = pc - __shfl(excl, o);  // < the fill of group o (0 where T = 0)
        const int32_t* lo = reinterpret_cast<const int32_t*>(
            reinterpret_cast<const char*>(lds_raw) + o * kGroupBytes + WIN * sizeof(WinRec));
        const int32_t s = lo[i];
        return ok ? s : slot0;
      };
      const bool has_prev = n > 0 && gb > 0, has_next = p0 + n < T && n > 0;
      const int32_t sp = pooled_slot(p0 - 1, has_prev), sn = pooled_slot(p0 + n, has_next);
      const int32_t cp = a.slots[sp].col, cn = a.slots[sn].col;
      head_open = has_prev;
      first_col = has_prev ? cp : -1;
      if (has_next) next_col = cn;
      fill = n;
      if (T > 0) run_list([&](int e) -> int32_t { return pooled_slot(p0 + e, e < fill); }, per);
      last_col = cur;
      tail_open = next_col == cur;
    }
  }
  if (!pooled) {
    if constexpr (!CH) fill = 0;  // (an overflowing workgroup lists again from the start)
#pragma unroll
    for (int u = 0; u < TRIPS; ++u) {
      unsigned long long word = wd[u];
      const int32_t s0 = slot0 + (u * LPR + l) * 64;  // first slot of this lane's word
      // move the trip's marked slots into the list in lane (= slot) order, as many as the list
      // has room for; when a group's list is full and it has marks left, every group of the
      // wave runs the chain on what it has listed so far
      while (__ballot(word != 0ull)) {
        const int cnt = __popcll(word);
        const int before = group_scan<LPR>(cnt, l) - cnt;  // marks of the group's earlier lanes
        const int take = min(cnt, max(WIN - fill - before, 0));
        int pos = fill + before;
        for (int i = 0; i < take; ++i) {
          list[pos++] = s0 + (__ffsll((long long)word) - 1);
          word &= word - 1ull;
        }
        int added = take;
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) added += __shfl_xor(added, o, LPR);
        fill += added;
        if (__ballot(word != 0ull)) run_list(own_slot, WIN);
      }
    }
    if (__ballot(fill > 0)) run_list(own_slot, WIN);
  }

  // ---- columns that run over several tasks / parts of this workgroup ----------------------
  // the last column of a tail-open task is still in `acc` (if it got any entry here); a
  // column that both comes in and goes on (the task lies inside it) counts as a head row
  const bool through = head_open && tail_open && first_col == last_col;
  // this group owns the combine of last_col: the column starts (or, for a piece of a very
  // long column, this workgroup's share of it starts) in this task
  const bool own = (tail_open && !through) || tk.part >= 0;
  bool own_acc = false;  // ... and holds entries of it in `acc`
  if (cur >= 0) {
    if (own && cur == last_col) {
      own_acc = true;
    } else {
      finish();
    }
  }
  if (head_open && l == 0) head[k + 2] = (head_done ? 1.0 : 0.0) + (through ? 2.0 : 0.0);
  if (!head_open && l == 0) head[k + 2] = 0.0;
  __syncthreads();
  if (own) {
    if (!own_acc) {
      // (pooled: only the first part of a piece without marks, which needs no row of V)
      acc.clear();
      if (!pooled) {
        vold = load_v_row<VEC>(c.V, last_col, k, f);
        load_acc_row(o, gold, last_col, k, f);
      }
    }
    bool any = own_acc;
    for (int g2 = gb + 1; g2 < GPB; ++g2) {
      const double* h2 = heads + g2 * (k + 3);
      const int fl = int(h2[k + 2]);
      if (fl & 1) {
        any = true;
        acc.add_row(h2, f, k);
      }
      if (!(fl & 2)) break;  // the column ends in that task
    }
    if (tk.part >= 0) {
      // a piece of a column longer than the workgroup's tasks: its sums for fm_finalize_kernel
      double* row = c.parts + int64_t(tk.part) * (k + 3);
      acc.store_row(row, f, k, scalars);
      if (scalars) row[k + 2] = any ? c.stamp : 0.0;
    } else if (any) {
      apply_column(c, o, last_col, acc, vold, gold, f, scalars);
    }
  }
}

// ---------------------------------------------------------------------------
// 3. columns split over several tasks: their partial rows, in slot order
// ---------------------------------------------------------------------------
struct FinArgs {
  ColArgs c;
  const SplitCol* split;  // [n_split_short | n_split_long]
  int32_t n_split_short;  // few partial rows: one lane group per column
  int32_t n_split_long;   // many partial rows: one workgroup per column
};

// The short split columns, one per lane group (workgroup b takes kBlock / LPR of them), the
// factors fb + lane * VEC on of each: the column's partial rows CB to a round of loads, read
// unconditionally -- a stale row is masked by its stamp -- and added in row order.
template <int LPR, int VEC, int CB, class O>
__device__ inline void finalize_short_columns(const FinArgs& a, const O& o, int b, int fb) {
  constexpr int GPB = kBlock / LPR;
  const ColArgs& c = a.c;
  const int k = c.k;
  const int l = threadIdx.x % LPR;
  const int ci = b * GPB + threadIdx.x / LPR;
  if (ci >= a.n_split_short) return;
  const SplitCol cc = a.split[ci];
  const int f = fb + l * VEC;
  const int fc = f < k ? f : 0;
  ColAcc<VEC> acc;
  acc.clear();
  const Pack<VEC> vold = load_v_row<VEC>(c.V, cc.col, k, f);
  Pack<VEC> gold;
  load_acc_row(o, gold, cc.col, k, f);
  bool any = false;
  for (int i = 0; i < cc.part_count; i += CB) {
    ColAcc<VEC> part[CB];
    double ss[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) {
      const double* row = c.parts + int64_t(cc.part_begin + (i + u < cc.part_count ? i + u : i)) * (k + 3);
      part[u].load_row(row, fc, k);
      ss[u] = row[k + 2];
    }
#pragma unroll
    for (int u = 0; u < CB; ++u) {
      const bool ok = i + u < cc.part_count && ss[u] == c.stamp;
      any = any || ok;
      acc.add_if(ok, part[u]);
    }
  }
  if (any) apply_column(c, o, cc.col, acc, vold, gold, f, l == 0 && fb == 0);
}

// blocks [0, nb_short): short split columns, one per lane group; then one block per long
// split column.  Launched only when the plan has split columns.
template <int LPR, int VEC, class O = SgdRule>
__global__ __launch_bounds__(kBlock) void fm_finalize_kernel(ArgsUnder<FinArgs, O> a, int nb_short) {
  const O& o = rule_of(a);
  __shared__ double scratch[kBlock];
  __shared__ double tot[1024 + 2];
  __shared__ int touched;
  const ColArgs& c = a.c;
  const int k = c.k;
  const int b = blockIdx.x;
  if (b < nb_short) return finalize_short_columns<LPR, VEC, 4>(a, o, b, 0);
  const SplitCol cc = a.split[a.n_split_short + (b - nb_short)];
  // is any partial row of this step's?  (an untouched column is left alone)
  if (threadIdx.x == 0) touched = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < cc.part_count; r += kBlock)
    if (c.parts[int64_t(cc.part_begin + r) * (k + 3) + k + 2] == c.stamp) touched = 1;
  __syncthreads();
  if (!touched) return;
  ordered_rows_sum<8>(PartRows{c.parts, cc.part_begin, k, c.stamp}, cc.part_count, k + 2, scratch, tot);
  apply_column_block(c, o, cc.col, tot);
}

// The same for factor counts of several chunks per lane, one chunk of 64 x VEC factors per
// workgroup (blockIdx.y), as fm_consume_kernel's CH form: a short column's partial rows (at
// most kShortSplit) are ONE round of loads, a long column's are summed by one thread per
// factor of the chunk with 32 rows in flight; stamps ride with the rows and the column's row of
// V is requested before the sums, so a workgroup's chain is two dependent levels instead of
// eight (k = 400, B = 2 000: 8.1 -> 6.8 us per launch, profiles/r3j vs r3q).
template <int VEC, class O = SgdRule>
__global__ __launch_bounds__(kBlock) void fm_finalize_chunk_kernel(ArgsUnder<FinArgs, O> a,
                                                                  int nb_short) {
  const O& o = rule_of(a);
  constexpr int CW = kWave * VEC;
  __shared__ double tot[CW + 2];
  const ColArgs& c = a.c;
  const int k = c.k;
  const int b = blockIdx.x;
  const int fb = int(blockIdx.y) * CW;
  if (b < nb_short) {
    // finalize_short_columns<kWave, VEC, kShortSplit>, open-coded: through the shared routine this
    // kernel measured 0.3 us slower at k = 400 (profiles/n11/bench_parent_vs_this.txt)
    constexpr int LPR = kWave;
    constexpr int GPB = kBlock / LPR;
    constexpr int CB = 8;
    const int l = threadIdx.x % LPR;
    const int ci = b * GPB + threadIdx.x / LPR;
    if (ci >= a.n_split_short) return;
    const SplitCol cc = a.split[ci];
    const int f = fb + l * VEC;
    const int fc = f < k ? f : 0;
    ColAcc<VEC> acc;
    acc.clear();
    Pack<VEC> vold;
    vold.load(c.V + int64_t(cc.col) * k + fc);
    Pack<VEC> gold;
    load_acc_row(o, gold, cc.col, k, f);
    bool any = false;
    for (int i = 0; i < cc.part_count; i += CB) {
      Pack<VEC> mm[CB];
      double gg[CB], dd[CB], ss[CB];
#pragma unroll
      for (int u = 0; u < CB; ++u) {
        const double* row = c.parts + int64_t(cc.part_begin + (i + u < cc.part_count ? i + u : i)) * (k + 3);
        mm[u].load(row + fc);
        gg[u] = row[k];
        dd[u] = row[k + 1];
        ss[u] = row[k + 2];
      }
#pragma unroll
      for (int u = 0; u < CB; ++u) {
        const bool ok = i + u < cc.part_count && ss[u] == c.stamp;
        any = any || ok;
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.m[v] += ok ? mm[u].v[v] : 0.0;
        acc.gw += ok ? gg[u] : 0.0;
        acc.d += ok ? dd[u] : 0.0;
      }
    }
    if (any) apply_column(c, o, cc.col, acc, vold, gold, f, l == 0 && fb == 0);
    return;
  }
  const SplitCol cc = a.split[a.n_split_short + (b - nb_short)];
  const int fcnt = k - fb < CW ? k - fb : CW;  // factors of this chunk
  const int j = threadIdx.x;                   // < fcnt: factor fb + j; fcnt, fcnt + 1: sum coef, sum coef * x
  const bool live = j < fcnt + 2;
  const int cidx = j < fcnt ? fb + j : k + (j - fcnt);
  const double vold = c.V[int64_t(cc.col) * k + (j < fcnt ? fb + j : 0)];
  double gold = 0.0;
  if constexpr (O::kAda) gold = o.acc_V[int64_t(cc.col) * k + (j < fcnt ? fb + j : 0)];
  double acc = 0.0;
  bool any = false;
  constexpr int U = 32;
  for (int r0 = 0; r0 < cc.part_count; r0 += U) {
    double v[U], st[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double* row = c.parts + int64_t(cc.part_begin + (r0 + u < cc.part_count ? r0 + u : r0)) * (k + 3);
      v[u] = row[live ? cidx : 0];
      st[u] = row[k + 2];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = r0 + u < cc.part_count && st[u] == c.stamp;
      any = any || ok;  // (the stamps are the same for every thread: uniform)
      acc += ok ? v[u] : 0.0;
    }
  }
  if (!any) return;  // an untouched column is left alone
  if (live) tot[j] = acc;
  __syncthreads();
  const double gw = tot[fcnt], d = tot[fcnt + 1];
  if (j < fcnt) {
    const int64_t at = int64_t(cc.col) * k + fb + j;
    if constexpr (O::kAda) {
      const double g = updated_factor(vold, acc, d, c.lr, true, false);
      c.V[at] = adagrad_element(vold, g, c.lr, o.eps, &gold);
      o.acc_V[at] = gold;
    } else if (c.grad)
      c.grad[at] = updated_factor(vold, acc, d, c.lr, true, false);
    else
      c.V[at] = updated_factor(vold, acc, d, c.lr, false, false);
  }
  if (j == 0 && fb == 0) {
    if constexpr (O::kAda) {
      apply_w(c, o, cc.col, gw);
    } else if (c.grad) {
      c.grad[c.n * k + cc.col] = -gw;
      if (c.touch) c.touch[cc.col] = c.touch_id;
    } else {
      add_by_only_writer(c.w + cc.col, c.lr * gw);
    }
  }
}

// RFM_CHECK_IDS=1: the row ids of one step must lie in the log and be distinct (a row's
// batch position is recorded with a plain store, so a repeated id would lose one of its
// contributions).  seen[r] holds the stamp of the last iteration that named row r.
__global__ __launch_bounds__(kBlock) void ids_check_kernel(const int32_t* ids, int64_t batch,
                                                          int64_t n_iters, int64_t n_rows,
                                                          int32_t* seen, int32_t stamp0,
                                                          int32_t* flags) {
  const int64_t total = batch * n_iters;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * kBlock) {
    const int32_t r = ids[i];
    const int32_t stamp = stamp0 + int32_t(i / batch);
    if (r < 0 || r >= n_rows) {
      atomicOr(&flags[0], 1);
    } else if (atomicExch(&seen[r], stamp) == stamp) {
      atomicOr(&flags[1], 1);
    }
  }
}

// theta -= lr * grad over [V | w | w0]
__global__ __launch_bounds__(kBlock) void fm_apply_kernel(double* V, double* w, double* w0,
                                                         const double* grad, int64_t nk,
                                                         int64_t n, double lr) {
  const int64_t total = nk + n + 1;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * kBlock) {
    double* dst = i < nk ? V + i : (i < nk + n ? w + (i - nk) : w0);
    *dst -= lr * grad[i];
  }
}

}  // namespace rfm
