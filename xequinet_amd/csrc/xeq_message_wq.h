// What the two halves of the wave / quad message kernels share (xeq_message_wq.hip: plan, records, weight packing, forward kernel;
// xeq_message_wq_bwd.hip: reverse kernel, edge gradients): the record layout and its bf16 split, the launch arguments and how a
// workgroup decodes its work, weight staging, the filter tile, the tile table and its row loads, the stamp instrument, the host-side
// checks and launch geometry, and the dispatch macros.  The walk order and the arithmetic mapping are described at the top of
// xeq_message_wq.hip.
#pragma once
#include "xeq_common.h"

namespace xeq {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// The filter contraction, split (round 3).  phi[e][ch] = sum_k rho~[e][k] W[ch][k] was K + 1 = 21 exact-f32 MFMA steps (11 x
// v_mfma_f32_32x32x2_f32 = 704 matrix-pipe cycles per 32 x 32 tile), and the tile loops of these kernels run within 80 % of that
// pipe bound (two waves share a SIMD's pipe; step timeline of round 3).  The f32 MFMA runs at 1/16 of the bf16 rate, so the first
// sixteen k now go through bf16 MFMAs on operands split three ways, x = hi + mid + lo with bf16 parts (8 + 8 + 8 significant
// bits, exact): six products hi hi, hi mid, mid hi, hi lo, lo hi, mid mid of v_mfma_f32_32x32x16_bf16 (32 cycles each, f32
// accumulate) leave out mid lo, lo mid, lo lo = 2^-24 of a product, the size of one f32 rounding; the remaining k (16 .. B - 1)
// and the bias column stay exact-f32 steps.  K = 21: 6 x 32 + 3 x 64 = 384 pipe cycles instead of 704.
// dwords per record: [kh][hi | mid | lo][4] bf16 packs of k = 8 kh .. 8 kh + 7 (24), [kh][TW] f32 tail (q = 2 s + kh -> k = 16 + q, then the
// envelope for the bias; TW = 4 tail values per k half up to 23 basis functions (KS <= 4 exact-f32 steps), 8 up to 31 (KS = 8)), Y1[3] Y2[5]:
// 40 dwords (160 B) or 48 (192 B)
// Round 6: the tail of up to FIVE values (k = 16 .. 19 and the bias column: num_basis <= 20, the default) runs through the bf16 matrix
// instruction as well.  A 16-slot k block holds the three splits of the five values, A = [hi_0..4 | mid_0..4 | lo_0..4 | 0], and is
// multiplied against THREE weight arrangements B1 = [hi | hi | hi | 0], B2 = [mid | mid | 0 | 0], B3 = [lo | 0 | 0 | 0] (packed once per
// weight version): A B1 + A B2 + A B3 = a_hi (b_hi + b_mid + b_lo) + a_mid (b_hi + b_mid) + a_lo b_hi, the same six products as the
// first sixteen k (what is left out is 2^-24 of a product).  Three 32-cycle instructions replace three 64-cycle exact-f32 steps: 288
// instead of 384 matrix-pipe cycles per filter tile; the record keeps its 160 bytes (the tail's eight floats become eight dwords of
// bf16 pairs).  Wider tails (num_basis 21 .. 31) keep the exact-f32 steps.
constexpr bool wq_bftail(int ks) { return ks <= 3; }
constexpr int WQ_TAIL = 24;                // dword offset of the tail inside a record
constexpr int wq_tailw(int ks) { return ks <= 4 ? 4 : 8; }
constexpr int wq_recf(int ks) { return WQ_TAIL + 2 * wq_tailw(ks) + 8; }
constexpr int wq_yoff(int ks) { return WQ_TAIL + 2 * wq_tailw(ks); }
// KS: 1 / 3 = a tail of up to 1 / 5 values (basis functions from k = 16 on, then the bias column) in the bf16 block (wq_bftail); from six
// values on, the exact-f32 steps of the tail, two values per step (never below 4, so that the two forms do not share a KS)
constexpr int wq_tail_values(int num_basis) { return (num_basis > 16 ? num_basis - 16 : 0) + 1; }
constexpr int wq_ks(int num_basis) {
  return wq_tail_values(num_basis) <= 1 ? 1 : (wq_tail_values(num_basis) <= 5 ? 3 : ((wq_tail_values(num_basis) + 1) / 2 < 4 ? 4 : (wq_tail_values(num_basis) + 1) / 2));
}
// xeq_edge_basis_wq lays the records out for wq_ks(num_basis) itself; the kernels that read them are instantiated for KS in {1, 3, 4, 8}
// only (wq_ks_template: 5, 6, 7 run as 8 on zero-filled tail positions).  Both must mean the same record for every step count.
static_assert(wq_tailw(5) == wq_tailw(8) && wq_tailw(6) == wq_tailw(8) && wq_tailw(7) == wq_tailw(8) && !wq_bftail(5) && !wq_bftail(8),
              "records written for 5, 6 or 7 tail steps are read by the KS = 8 kernels");
constexpr int WQ_REC_MAX = 48;
static_assert(wq_recf(8) == WQ_REC_MAX && wq_recf(4) == 40 && wq_recf(1) == wq_recf(4) && wq_recf(3) == wq_recf(4), "record widths of include/xeq.h");
__device__ __forceinline__ uint32_t wq_bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// x = hi + mid + lo, each a bf16 (round to nearest even of what is left): returns the three 16-bit patterns
__device__ __forceinline__ void wq_split3(float x, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
  hi = wq_bf16_rne(x);
  const float r1 = x - __uint_as_float(hi << 16);
  mid = wq_bf16_rne(r1);
  const float r2 = r1 - __uint_as_float(mid << 16);
  lo = wq_bf16_rne(r2);
}
// value at tail position q of a record / weight row: k = 16 + q while k < B, then the bias column, then zeros
__device__ __forceinline__ int wq_tail_k(int q, int B) { return 16 + q < B ? 16 + q : (16 + q == (B > 16 ? B : 16) ? -1 : -2); }
constexpr uint32_t WQ_FIRST = 1u << 30, WQ_LAST = 1u << 31, WQ_OWNER = (1u << 30) - 1u;
#ifndef XEQ_WQ_WAVES
#define XEQ_WQ_WAVES 4
#endif
constexpr int WQ_WAVES = XEQ_WQ_WAVES;     // waves per workgroup: they share the unit's weights and, step by step, the window

// ------------------------------------------------------------------------------------------------ common
struct WqArgs {
  int64_t n_nodes, n_edges, pcap;
  int n_ranges;
  const int32_t* sq;       // [2 R + 1] quad boundaries of the streams (range w: streams 2w and 2w + 1)
  const int32_t* sn;       // [2 R + 1] node boundaries of the streams
  const int32_t* rowptr;   // [N + 1] CSR of the walk order (isolated nodes)
  const int32_t* pgath;    // [P] gathered node per padded slot
  const uint32_t* qinfo;   // [Q] owner | WQ_FIRST | WQ_LAST per quad
  const int32_t* win;      // [2 n_steps(1)] window (first node, rows) of every step of the SHORT class, then [2 n_steps(mlong)] of the long class
  // Stream classes (round 6).  The stream table (sq, sn) holds SHORT streams; the l = 0 units walk LONG streams, each `mlong` consecutive
  // table streams (1: one class, as up to round 5).  Why: the l > 0 units gather 5-7 pieces of 128 bytes per window row, so their steps
  // must stay short for the window to fit LDS (a step that does not fit gathers from global memory: the l = 2 unit's forward launch alone
  // 90 us at 48 edges per stream, 148 us at 80), while the l = 0 units -- 2-4 pieces per row, more than half of the work -- run fastest on
  // long streams (fewer range prologues, window stagings and barriers per edge).  The work of a workgroup is cut in UNITS of `mlong`
  // short steps = one long step, so that the units of one chunk still walk the same records at about the same time.
  int mlong;
  int n_steps, steps_per_wg;   // in chunk UNITS (see above); steps_per_wg: units of a LONG chunk
  int regions, region_steps;   // the units are cut in `regions` contiguous regions (one per XCD when the grid is XCD-mapped)
  int lvl_chunks[3], lvl_spw[3], lvl_start[3];   // per region: three runs of chunks, long to short (chunks, steps per chunk, first
                                                 // step): the grid ends on short workgroups (a region's last chunks start last)
  int F, C, D, H, B;
  Irreps ir;
  int xl;                  // layout of xhat / grad_xhat
  int mirror;              // reverse pass over the FORWARD plan of a symmetric list: every slot stands for its mirror edge (Y_1 negated)
  int packed_w;            // w_rbf points at xeq_message_wq_pack_weights' output (XEQ_WQ_PACKED_WEIGHTS): staging is a coalesced copy
  int nu[3];               // 32-channel units per l
  // table form of the first block (TAB below): h / xhat of a node are rows of the element table.  Forward: pgath points at the table
  // row of every slot's gathered node; reverse: qtab holds the table row of every quad's owner
  const int32_t* qtab;     // [Q]
  int tab_rows;            // rows of the table (T)
};

struct WqUnit {
  int l, cb, u0, xbase;
};
__device__ __forceinline__ WqUnit wq_unit(const WqArgs& a, int u) {
  WqUnit w;
  if (u < a.nu[0]) {
    w.l = 0;
    w.cb = u;
  } else if (u < a.nu[0] + a.nu[1]) {
    w.l = 1;
    w.cb = u - a.nu[0];
  } else {
    w.l = 2;
    w.cb = u - a.nu[0] - a.nu[1];
  }
  const int cbase = w.l == 0 ? 0 : (w.l == 1 ? a.ir.mul[0] : a.ir.mul[0] + a.ir.mul[1]);
  w.u0 = cbase + 32 * w.cb;
  int l_, off;
  a.ir.locate(w.u0, l_, off);
  w.xbase = off;
  return w;
}

// the stream class of a unit: multiplier, ranges and steps of the class, its window table
struct WqClass {
  int m, n_ranges, n_steps;
  const int32_t* win;
};
__host__ __device__ __forceinline__ int wq_class_steps(int n_ranges, int m) { return ((n_ranges + m - 1) / m + WQ_WAVES - 1) / WQ_WAVES; }
__device__ __forceinline__ WqClass wq_class(const WqArgs& a, int l) {
  WqClass c;
  c.m = (l == 0) ? a.mlong : 1;
  c.n_ranges = (a.n_ranges + c.m - 1) / c.m;
  c.n_steps = wq_class_steps(a.n_ranges, c.m);
  c.win = (l == 0 && a.mlong > 1) ? a.win + 2 * wq_class_steps(a.n_ranges, 1) : a.win;
  return c;
}
// Per-l builds (the other units exit) say the units want different stream lengths (QM9-1024,
// us per launch at 48 / 64 / 80 / 112 / 160 edges per stream: forward l = 0 93 / 87 / 79 / 86 / 81, l = 1 65 / 64 / 76 / 89 / 131, l = 2
// 90 / 109 / 148 / 147 / 157; reverse l = 0 171 / 157 / 145 / 163 / 134, l = 1 102 / 96 / 109 / 96 / 117, l = 2 122 / 113 / 136 / 157 / 190;
// profiles/r06_small_experiments.txt item 6) -- but see below.
// MEASURED AND SWITCHED OFF (round 6, profiles/r06_small_experiments.txt item 6): with all seven units in one launch the classes LOSE --
// QM9-1024, whole step, one box: one class of 80 edges 1.731 ms | 48 x 3 1.775 | 48 x 2 1.790 | 64 x 2 1.747 | 40 x 3 1.796 | one class of
// 48 1.838.  A unit alone on the chip is a latency measurement (290 workgroups, one or two per CU); seven units together are a throughput
// measurement, and there every additional step (barrier, staging, range prologue) of the l > 0 units costs more than their window misses.
// The mechanism stays behind XEQ_WQ_LONG_MULT (development; results do not depend on it, tests/test_gpu_parity.py) with one class as default.
static int wq_long_mult(int64_t n_edges, int n_ranges) {
  const char* env = getenv("XEQ_WQ_LONG_MULT");
  if (env && atoi(env) >= 1 && atoi(env) <= 8) return atoi(env);
  (void)n_edges;
  (void)n_ranges;
  return 1;
}

// Work of a workgroup: (chunk of consecutive steps, unit).  A step is WQ_WAVES consecutive ranges, one per wave; the
// waves share the unit (its rbf_lin rows, staged once in LDS) and, step by step, the window of gathered node rows.
// Consecutive work items are the units of one chunk (they share its records and index arrays) and are dealt to
// workgroups so that they run on one XCD (blocks b and b + 8 share one under round-robin dispatch: speed only).
__device__ __forceinline__ void wq_decode(const WqArgs& a, int nunits, int& s0, int& s1, int& unit) {
  const int b = blockIdx.x;
  int region, j;   // region and item index inside it
  if (a.regions == 8) {
    region = b & 7;
    j = b >> 3;
  } else {
    region = 0;
    j = b;
  }
  const int c = j / nunits;   // chunk inside the region
  unit = nunits - 1 - (j - c * nunits);   // a chunk's l = 2 unit first, its l = 0 units last
  const int base = region * a.region_steps, rend = min(base + a.region_steps, a.n_steps);
  s0 = s1 = 0;   // padding block of the grid: no steps
  int cc = c;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    if (cc >= 0 && cc < a.lvl_chunks[v]) {
      const int lend = v < 2 ? base + a.lvl_start[v + 1] : rend;
      s0 = base + a.lvl_start[v] + cc * a.lvl_spw[v];
      s1 = min(s0 + a.lvl_spw[v], min(lend, rend));
    }
    cc -= a.lvl_chunks[v];
  }
}

// The window of a step in LDS: rows [w0, w0 + rows) of the gathered node arrays, restricted to the unit's columns, as
// NSL pieces of 128 bytes per row.  Staged with 16-byte loads (8 lanes per piece), read back per row with 4-byte LDS
// reads: a 64-lane dword load from global memory occupies the CU's texture addresser as long as a 16-byte one
// (16 cycles), so the per-row gathers -- 92 per tile on average -- bound the older forms (MI355X: 1 750 cycles per
// tile and CU measured, against 450 for the MFMAs); out of LDS the same reads cost 2 cycles each.
#ifndef XEQ_WQ_WIN_FLOATS
#define XEQ_WQ_WIN_FLOATS 12288
#endif
constexpr int WQ_WIN_FLOATS = XEQ_WQ_WIN_FLOATS;   // 48 KB per workgroup: two workgroups per CU
// rows of the element table the forward table form can hold next to nothing else in the window's LDS (its l = 0 rows: 512 bytes)
constexpr int WQ_TAB_MAX_ROWS = WQ_WIN_FLOATS * 4 / 512 < 128 ? WQ_WIN_FLOATS * 4 / 512 : 128;

// rbf_lin rows of the unit as the B operands, per kind (0: gate_state, 1: gate_edge, 2: scalar message) WQ_WK<KS> floats:
//   [split][lane][4]   bf16 packs of W[row][8 kh + j], j = 0..7 (lane: j = lane & 31 -> channel row, kh = lane >> 5); 3 x 64 x 4
//   [s][lane]          f32 tail: position q = 2 s + kh (wq_tail_k: k = 16 + q, then the bias, then zeros); KS x 64
//   wq_bftail(KS): instead of the f32 tail [arrangement v][lane][4]: bf16 packs of slots 8 kh .. 8 kh + 7 of B1 / B2 / B3 (above); 3 x 64 x 4
template <int KS>
constexpr int WQ_WK = 3 * 64 * 4 + (wq_bftail(KS) ? 3 * 64 * 4 : KS * 64);
template <int KS>
__device__ __forceinline__ void wq_stage_weights(const WqArgs& a, const WqUnit& un, const float* __restrict__ w,
                                                 const float* __restrict__ b, float* wl) {
  const int nkind = un.l == 0 ? 3 : 2, B = a.B;
  if (a.packed_w) {   // the unit's block of the packed copy, already in this layout: 16-byte coalesced loads (round 5)
    const int unit_index = (un.l == 0 ? 0 : (un.l == 1 ? a.nu[0] : a.nu[0] + a.nu[1])) + un.cb;
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(w + (size_t)unit_index * (3 * WQ_WK<KS>));
    for (int idx = threadIdx.x; idx < nkind * WQ_WK<KS> / 4; idx += blockDim.x) reinterpret_cast<f32x4*>(wl)[idx] = src[idx];
    return;
  }
  auto row_of = [&](int kind, int ln) { return (kind == 0 ? un.u0 : (kind == 1 ? a.C + un.u0 : 2 * a.C + 32 * un.cb)) + (ln & 31); };
  for (int idx = threadIdx.x; idx < nkind * 3 * 64; idx += blockDim.x) {   // one 16-byte pack per thread and trip
    const int kind = idx / 192, rem = idx - 192 * kind, split = rem >> 6, ln = rem & 63;
    const int row = row_of(kind, ln), kh = ln >> 5;
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int k = 8 * kh + jj;
      uint32_t a3[3];
      wq_split3(k < B ? w[(int64_t)row * B + k] : 0.f, a3[0], a3[1], a3[2]);
      pk[jj >> 1] |= a3[split] << (16 * (jj & 1));
    }
    *reinterpret_cast<f32x4*>(wl + kind * WQ_WK<KS> + 4 * (64 * split + ln)) =
        f32x4{__uint_as_float(pk[0]), __uint_as_float(pk[1]), __uint_as_float(pk[2]), __uint_as_float(pk[3])};
  }
  if constexpr (wq_bftail(KS)) {
    for (int idx = threadIdx.x; idx < nkind * 3 * 64; idx += blockDim.x) {   // one 16-byte pack per thread and trip
      const int kind = idx / 192, rem = idx - 192 * kind, v = rem >> 6, ln = rem & 63;
      const int row = row_of(kind, ln), kh = ln >> 5;
      uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int slot = 8 * kh + jj, part = slot / 5, q = slot - 5 * part;   // slot 15: padding
        const int k = wq_tail_k(q, B);
        uint32_t a3[3];
        wq_split3(k >= 0 ? w[(int64_t)row * B + k] : (k == -1 ? b[row] : 0.f), a3[0], a3[1], a3[2]);
        // arrangement v multiplies the record's part `part` (0 hi, 1 mid, 2 lo) by the weight's split v, where part + v <= 2
        const uint32_t val = (slot < 15 && part + v <= 2) ? a3[v] : 0u;
        pk[jj >> 1] |= val << (16 * (jj & 1));
      }
      *reinterpret_cast<f32x4*>(wl + kind * WQ_WK<KS> + 768 + 4 * (64 * v + ln)) =
          f32x4{__uint_as_float(pk[0]), __uint_as_float(pk[1]), __uint_as_float(pk[2]), __uint_as_float(pk[3])};
    }
    return;
  }
  for (int idx = threadIdx.x; idx < nkind * KS * 64; idx += blockDim.x) {
    const int kind = idx / (KS * 64), rem = idx - kind * (KS * 64), sstep = rem >> 6, ln = rem & 63;
    const int row = row_of(kind, ln), k = wq_tail_k(2 * sstep + (ln >> 5), B);
    wl[kind * WQ_WK<KS> + 768 + rem] = k >= 0 ? w[(int64_t)row * B + k] : (k == -1 ? b[row] : 0.f);
  }
}

// what a lane holds of the record of the MFMA row it owns: the three bf16 packs of its eight k and KS tail values
template <int KS>
struct WqR {
  f32x4 b[3];
  float f[wq_bftail(KS) ? 4 : KS];   // wq_bftail: the four dwords of the lane's eight tail slots
};
// W: the kind's block of the staged weights, + 4 lane for the packs / + 768 + lane for the tail (wq_wptr)
template <int KS>
__device__ __forceinline__ f32x16 wq_filter(const WqR<KS>& R, const float* W, int lane) {
  f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const f32x4* Wb = reinterpret_cast<const f32x4*>(W) + lane;
  const bf16x8 ah = __builtin_bit_cast(bf16x8, R.b[0]), am = __builtin_bit_cast(bf16x8, R.b[1]), al = __builtin_bit_cast(bf16x8, R.b[2]);
  const bf16x8 bh = __builtin_bit_cast(bf16x8, Wb[0]), bm = __builtin_bit_cast(bf16x8, Wb[64]), bl = __builtin_bit_cast(bf16x8, Wb[128]);
  // small terms first
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, d, 0, 0, 0);
  if constexpr (wq_bftail(KS)) {   // the tail block against its three weight arrangements, smallest first (a_hi b_lo | a (b_mid) | a (b_hi))
    const f32x4 tv = {R.f[0], R.f[1], R.f[2], R.f[3]};
    const bf16x8 at = __builtin_bit_cast(bf16x8, tv);
    const f32x4* Wt = reinterpret_cast<const f32x4*>(W + 768) + lane;
    const bf16x8 t1 = __builtin_bit_cast(bf16x8, Wt[0]), t2 = __builtin_bit_cast(bf16x8, Wt[64]), t3 = __builtin_bit_cast(bf16x8, Wt[128]);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, t3, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, t2, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, t1, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, d, 0, 0, 0);
    return d;
  }
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, d, 0, 0, 0);
  const float* Wf = W + 768 + lane;
#pragma unroll
  for (int s = 0; s < KS; ++s) d = __builtin_amdgcn_mfma_f32_32x32x2f32(R.f[s], Wf[s * 64], d, 0, 0, 0);
  return d;
}

__device__ __forceinline__ float wq_ld(const float* __restrict__ base, uint32_t byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ void wq_st(float* __restrict__ base, uint32_t byte_off, float v) {
  *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// The tile table (LDS, private to the wave, double-buffered).  Position p = 16 * half + v is row v of that half's
// stream in this tile (v = accumulator register); quad slot c = 4 * half + g.
//   [T_G0 + p], [T_G1 + p]      byte offsets of the row's two gathered node rows
//   [T_Y + 32 m + p]            Y_lm of the row (m = 0..2: Y_1, 3..7: Y_2)
//   [T_QOWN + c]                owner node of the quad
//   [T_QKEEP + c]               0 where the quad starts a segment (running sums restart), else 1
//   [T_QLAST + c]               1 where the quad ends a segment (the node's sums are stored)
//   [T_QTAB + c]                table form of the reverse pass: the owner's row of the element table
enum { T_G0 = 0, T_G1 = 32, T_Y = 64, T_QOWN = 320, T_QKEEP = 328, T_QLAST = 336, T_QTAB = 344, T_SIZE = 352 };

// what a lane loads for the MFMA row it owns: i = lane & 31 -> half hr = (i >> 2) & 1, register v = 4 (i >> 3) + (i & 3)
template <int KS, int NREC, bool WITH_Y>
struct WqRow {
  WqR<KS> R[NREC];
  f32x4 ya, yb;
  int g;
  uint32_t qi;
  int qt;   // (QTAB only)
};
struct WqStreams {
  int q0, q1, q2, ntiles;
};
// Rows beyond the stream's end (`valid` false) read slot 0's record as it stands (round 6; they used to be zeroed, 38 selects per tile
// and lane in the reverse kernel): their quad carries neither the FIRST nor the LAST flag and comes behind the stream's last real quad
// -- whose LAST flag has stored the node's sums --, so whatever such a row adds to the running sums is never stored, and the per-edge
// partials of the reverse pass are stored for slots inside the stream only (`keeper`).
template <int KS>
__device__ __forceinline__ void wq_load_rec(const float* __restrict__ rec, uint32_t ps, int kh, bool valid, WqR<KS>& R) {
  const f32x4* __restrict__ rp = reinterpret_cast<const f32x4*>(rec + (size_t)ps * wq_recf(KS) + 12 * kh);
#pragma unroll
  for (int c = 0; c < 3; ++c) R.b[c] = rp[c];
  const f32x4* __restrict__ tp = reinterpret_cast<const f32x4*>(rec + (size_t)ps * wq_recf(KS) + WQ_TAIL + wq_tailw(KS) * kh);
#pragma unroll
  for (int c = 0; c < wq_tailw(KS) / 4; ++c) {
    const f32x4 tl = tp[c];
#pragma unroll
    for (int s = 4 * c; s < 4 * c + 4; ++s)
      if (s < (wq_bftail(KS) ? 4 : KS)) R.f[s] = tl[s - 4 * c];
  }
}
template <int KS, int NREC, bool WITH_Y, bool QTAB = false>
__device__ __forceinline__ void wq_row(const WqArgs& a, const WqStreams& st, int lane, int t, const float* __restrict__ rec,
                                       const float* __restrict__ drec, WqRow<KS, NREC, WITH_Y>& w, int g_default = 0) {
  const int i = lane & 31, kh = lane >> 5, hr = (i >> 2) & 1, g = i >> 3;
  const int qb = hr ? st.q1 : st.q0, qe = hr ? st.q2 : st.q1;
  const int q = qb + 4 * t + g;
  const bool valid = q < qe;
  // invalid rows (beyond the stream's end) read slot 0 / quad 0 -- always in bounds -- and are then zeroed: no load sits
  // behind a branch, so the waits of the tile loop stay counted
  const uint32_t ps = valid ? 4u * (uint32_t)q + (uint32_t)(i & 3) : 0u;
  const int gv = a.pgath[ps];
  const uint32_t qv = a.qinfo[valid ? q : 0];
  w.g = valid ? gv : g_default;
  w.qi = valid ? qv : 0u;
  if constexpr (QTAB) w.qt = a.qtab[valid ? q : 0];   // (an invalid row's quad is never multiplied into a stored sum: any row of the table will do)
  wq_load_rec<KS>(rec, ps, kh, valid, w.R[0]);
  if constexpr (NREC > 1) wq_load_rec<KS>(drec, ps, kh, valid, w.R[1]);
  if constexpr (WITH_Y) {
    const float* __restrict__ ysrc = NREC > 1 ? drec : rec;   // (both records carry Y)
    const f32x4* __restrict__ yp = reinterpret_cast<const f32x4*>(ysrc + (size_t)ps * wq_recf(KS) + wq_yoff(KS));
    w.ya = yp[0];
    w.yb = yp[1];
    if (a.mirror) {   // the mirror edge's vector is the negative of the slot's: d and Y_2 are the same bits, Y_1 changes sign
      w.ya[0] = -w.ya[0];
      w.ya[1] = -w.ya[1];
      w.ya[2] = -w.ya[2];
    }
  }
}
template <int KS, int NREC, bool WITH_Y, bool QTAB = false>
__device__ __forceinline__ void wq_publish(int lane, const WqRow<KS, NREC, WITH_Y>& w, uint32_t stride0, uint32_t stride1,
                                           int* tbl, uint32_t gbase = 0u) {
  // EVERY lane writes, without a branch (round 6).  Lanes l and l + 32 hold the same row (wq_row: i = lane & 31) and the four lanes of
  // a quad the same quad record, so the duplicates store equal values to equal addresses.  Why: behind `if (lane < 32)` / `if ((i & 3)
  // == 0)` the compiler SANK the index loads of wq_row (pgath, qinfo: requested a tile ahead in the source) into the branches that
  // alone use them -- two dependent global round trips per tile, each behind an s_waitcnt vmcnt(0) that also drained the record
  // prefetch (the forward kernel's l = 0 waves: 19.5 % of their cycles waiting for the record and 3.7 % at the publish by the stamps).
  const int i = lane & 31, hr = (i >> 2) & 1, v = 4 * (i >> 3) + (i & 3), p = 16 * hr + v;
  // (what the gathers cost, measured with every gather reading node 0: profiles/r02_wq_ablation.txt)
  tbl[T_G0 + p] = (int)(((uint32_t)w.g - gbase) * stride0);   // window mode: gbase = first row of the window
  tbl[T_G1 + p] = (int)(((uint32_t)w.g - gbase) * stride1);
  if constexpr (WITH_Y) {
    float* tf = reinterpret_cast<float*>(tbl);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      tf[T_Y + 32 * q + p] = w.ya[q];
      tf[T_Y + 32 * (4 + q) + p] = w.yb[q];
    }
  }
  const int c = 4 * hr + (i >> 3);
  tbl[T_QOWN + c] = (int)(w.qi & WQ_OWNER);
  tbl[T_QKEEP + c] = (w.qi & WQ_FIRST) ? 0 : 1;
  tbl[T_QLAST + c] = (w.qi & WQ_LAST) ? 1 : 0;
  if constexpr (QTAB) tbl[T_QTAB + c] = w.qt;
}
template <typename T>
__device__ __forceinline__ void wq_tread4(const int* tbl, int idx, T (&out)[4]) {
  static_assert(sizeof(T) == 4, "table entries are dwords");
  typedef T vec4 __attribute__((ext_vector_type(4)));
  const vec4 v = *reinterpret_cast<const vec4*>(reinterpret_cast<const T*>(tbl) + idx);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = v[i];
}

// per-lane byte columns of the unit
struct WqCols {
  uint32_t b_hs, b_hm, b_s, b_xe, b_x, xnode_b, xcomp_b;
  int64_t x_base;
};
template <int NM>
__device__ __forceinline__ WqCols wq_cols(const WqArgs& a, const WqUnit& un, int j) {
  WqCols w;
  const XAddr xa = xaddr(a.ir, a.n_nodes, un.u0, a.xl);
  w.b_hs = 4u * (uint32_t)(un.u0 + j);
  w.b_hm = 4u * (uint32_t)(2 * a.C + 32 * un.cb + j);
  w.b_s = 4u * (uint32_t)(32 * un.cb + j);
  w.b_xe = 4u * (uint32_t)(un.xbase + j * NM);
  w.b_x = 4u * (uint32_t)(j * (a.xl == 0 ? NM : 1));
  w.xnode_b = 4u * (uint32_t)xa.node;
  w.xcomp_b = 4u * (uint32_t)xa.comp;
  w.x_base = xa.off;
  return w;
}
__device__ __forceinline__ WqStreams wq_streams(const WqArgs& a, int range, int m = 1) {
  WqStreams s;
  const int last = 2 * a.n_ranges;   // (a class stream is m consecutive table streams; the last range of a class may be short)
  s.q0 = a.sq[min(2 * range * m, last)];
  s.q1 = a.sq[min((2 * range + 1) * m, last)];
  s.q2 = a.sq[min((2 * range + 2) * m, last)];
  const int l0 = s.q1 - s.q0, l1 = s.q2 - s.q1;
  s.ntiles = ((l0 > l1 ? l0 : l1) + 3) >> 2;
  return s;
}
// owner nodes of the wave's two streams that have no edge: fn(node) is called by all 64 lanes
// (nodes without an edge own a quad of padding slots since round 3 -- QuadCount, xeq_message_wq.hip -- and take the ordinary path; nothing to do here)
template <typename Fn>
__device__ __forceinline__ void wq_for_isolated(const WqArgs&, int, int, Fn) {}

// development (-DXEQ_WQ_STAMPS): cycles of the l = 0 waves per phase of the forward kernel, summed over a launch
static __device__ unsigned long long g_wq_stamps[32];   // (static: each of the two objects has its own)
static __device__ unsigned long long g_wq_wg[8192 * 4];   // -DXEQ_WQ_ROLE_TIME / _FWD: per workgroup of the reverse / forward kernel (hw id | l << 32, xcc id, start, end in 100 MHz ticks)
#ifdef XEQ_WQ_STAMPS
#define WQ_STAMP(i)                                                                                          \
  do {                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    unsigned long long now_;                                                                                 \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");                            \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    st_[i] += now_ - last_;                                                                                  \
    last_ = now_;                                                                                            \
  } while (0)
#else
#define WQ_STAMP(i) \
  do {              \
  } while (0)
#endif
// read and clear this object's counters (behind the debug entry points of either file)
static int wq_debug_wg(unsigned long long* out) {   // -DXEQ_WQ_ROLE_TIME / _FWD: 8192 x 4
  static unsigned long long zero[8192 * 4];
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wq_wg), sizeof(zero)) != hipSuccess) return XEQ_ERR_LAUNCH;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wq_wg), zero, sizeof(zero)) != hipSuccess) return XEQ_ERR_LAUNCH;
  return XEQ_OK;
}
static int wq_debug_stamps(unsigned long long out[32]) {   // -DXEQ_WQ_STAMPS: the phase cycle counters
  unsigned long long zero[32] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wq_stamps), sizeof(zero)) != hipSuccess) return XEQ_ERR_LAUNCH;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wq_stamps), zero, sizeof(zero)) != hipSuccess) return XEQ_ERR_LAUNCH;
  return XEQ_OK;
}

__device__ __forceinline__ float wq_lds(const float* win, uint32_t byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(win) + byte_off);
}

static bool wq_supported(int num_basis, int node_dim, const int32_t mul[3]) {
  return num_basis >= 1 && num_basis <= 31 && mul[0] == node_dim && mul[0] > 0 && mul[0] % 32 == 0 && mul[1] >= 0 &&
         mul[1] % 32 == 0 && mul[2] >= 0 && mul[2] % 32 == 0;
}
// padded slots: at most deg + 3 per node that has an edge, four per node that has none; the capacity every buffer of a plan is sized for
static int64_t wq_pcap(int64_t n_nodes, int64_t n_edges) { return (n_edges + 4 * n_nodes + 3) / 4 * 4; }
// 32-bit byte offsets: rows of h (n_nodes * H * 4) and records (pcap * 128)
static bool wq_fits(int64_t n_nodes, int64_t n_edges, int node_dim, const int32_t mul[3]) {
  const int64_t H = node_dim + 2 * (int64_t)(mul[0] + mul[1] + mul[2]);
  return n_nodes >= 0 && n_edges >= 0 && n_nodes * H * 4 < (1ll << 32) && wq_pcap(n_nodes, n_edges) * (int64_t)WQ_REC_MAX * 4 < (1ll << 32);
}

static int wq_check(const char* who, int64_t n_nodes, int64_t n_edges, int n_ranges, int num_basis, int node_dim,
                    const int32_t mul[3], WqArgs& a) {
  XEQ_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_edges < (1ll << 31) && n_nodes < (1ll << 30), "%s: bad sizes", who);
  XEQ_CHECK_ARG(n_ranges >= 1, "%s: the stream table must cover every node (n_ranges >= 1)", who);
  if (!wq_supported(num_basis, node_dim, mul)) {
    xeq::set_error("%s: the wave / quad form needs node_dim == mul[0], multiplicities in multiples of 32 and num_basis <= 31", who);
    return XEQ_ERR_UNSUPPORTED;
  }
  XEQ_CHECK_ARG(wq_fits(n_nodes, n_edges, node_dim, mul), "%s: tensors too large for 32-bit byte offsets (shard the batch)", who);
  for (int l = 0; l < 3; ++l) a.ir.mul[l] = mul[l];
  a.C = a.ir.C();
  a.D = a.ir.D();
  a.F = node_dim;
  a.H = a.F + 2 * a.C;
  a.B = num_basis;
  for (int l = 0; l < 3; ++l) a.nu[l] = mul[l] / 32;
  a.n_nodes = n_nodes;
  a.n_edges = n_edges;
  a.pcap = wq_pcap(n_nodes, n_edges);
  a.n_ranges = n_ranges;
  return XEQ_OK;
}

// Steps (WQ_WAVES ranges each) a workgroup walks.  Long chunks sized for ~6 workgroups per CU and unit mix over the first 70 % of a
// region's steps, then chunks a third as long: a launch is 5-6 workgroups per CU, each 100-190 us long (the l = 2 unit of a chunk
// runs 1.8x its l = 0 units), and with equal chunks the CUs finished between 300 and 457 us of a 457 us launch (QM9-1024 reverse
// pass, workgroup timeline); the short chunks fill that ragged end.  Regions keep the XCD mapping: block b runs on XCD b % 8 under
// round-robin dispatch (speed only), so region b % 8 is one XCD's contiguous share of the walk and ITS last chunks are the short ones.
static void wq_geometry(WqArgs& a, int nunits, unsigned& grid) {
  a.mlong = wq_long_mult(a.n_edges, a.n_ranges);
  a.n_steps = wq_class_steps(a.n_ranges, a.mlong);   // chunk units: one long step = mlong short steps
  const int64_t want_chunks = (256 * 6 + nunits - 1) / nunits;
  a.steps_per_wg = (int)((a.n_steps + want_chunks - 1) / want_chunks);
  if (a.steps_per_wg < 1) a.steps_per_wg = 1;
  const double frac = 0.8, frac2 = 0.2;   // (swept, with the steps per workgroup: profiles/r05_in_flight.txt)
  const int div = 3;
  const int64_t plain_blocks = (int64_t)((a.n_steps + a.steps_per_wg - 1) / a.steps_per_wg) * nunits;
  a.regions = plain_blocks >= 64 ? 8 : 1;
  a.region_steps = (a.n_steps + a.regions - 1) / a.regions;
  const int spw[3] = {a.steps_per_wg, a.steps_per_wg / div < 1 ? 1 : a.steps_per_wg / div, 1};
  const double share[3] = {frac, frac2, 1.0};
  int start = 0;
  for (int v = 0; v < 3; ++v) {
    a.lvl_spw[v] = spw[v];
    a.lvl_start[v] = start;
    int chunks = v < 2 ? (int)(share[v] * a.region_steps / spw[v]) : (a.region_steps - start + spw[v] - 1) / spw[v];
    if (start + (int64_t)chunks * spw[v] > a.region_steps) chunks = (a.region_steps - start + spw[v] - 1) / spw[v];
    if (chunks < 0) chunks = 0;
    a.lvl_chunks[v] = chunks;
    start += chunks * spw[v];
    if (start > a.region_steps) start = a.region_steps;
  }
  grid = (unsigned)((int64_t)a.regions * (a.lvl_chunks[0] + a.lvl_chunks[1] + a.lvl_chunks[2]) * nunits);
}

}  // namespace xeq

// KS: exact-f32 steps of the filter's tail -- the basis functions from k = 16 on and the bias column, two per step
#define XEQ_WQ_DISPATCH_KS(KERNEL, FLAG, ...)                                                                                \
  do {                                                                                                                       \
    const int ks = wq_ks(num_basis);                                                                                         \
    if (ks <= 1) hipLaunchKernelGGL((KERNEL<1, FLAG>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__);      \
    else if (ks <= 3) hipLaunchKernelGGL((KERNEL<3, FLAG>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__); \
    else if (ks <= 4) hipLaunchKernelGGL((KERNEL<4, FLAG>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<8, FLAG>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__);              \
  } while (0)
#define XEQ_WQ_DISPATCH(KERNEL, flag, ...)                   \
  do {                                                       \
    if (flag) XEQ_WQ_DISPATCH_KS(KERNEL, true, __VA_ARGS__); \
    else XEQ_WQ_DISPATCH_KS(KERNEL, false, __VA_ARGS__);     \
  } while (0)

// the table form of the first block: KERNEL<KS, true, true>
#define XEQ_WQ_DISPATCH_TAB(KERNEL, ...)                                                                                    \
  do {                                                                                                                      \
    const int ks = wq_ks(num_basis);                                                                                        \
    if (ks <= 1) hipLaunchKernelGGL((KERNEL<1, true, true>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__);      \
    else if (ks <= 3) hipLaunchKernelGGL((KERNEL<3, true, true>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__); \
    else if (ks <= 4) hipLaunchKernelGGL((KERNEL<4, true, true>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<8, true, true>), grid, dim3(64 * WQ_WAVES), 0, (hipStream_t)stream, __VA_ARGS__);              \
  } while (0)
// what the table entry points ask of their arguments (include/xeq.h: the callers ask xeq_message_wq_first_table first)
#define XEQ_WQ_CHECK_TABLE(who, rows, tab, hint)                                                                                  \
  do {                                                                                                                            \
    XEQ_CHECK_ARG((rows) >= 1 && (rows) <= WQ_TAB_MAX_ROWS, who ": the element table has %lld rows, the table form takes 1 .. %d", \
                  (long long)(rows), WQ_TAB_MAX_ROWS);                                                                            \
    XEQ_CHECK_ARG((tab) != nullptr && h_table != nullptr && xhat0_table != nullptr, who ": NULL table argument");                 \
    XEQ_CHECK_ARG(((hint) & 1) && ((hint) & XEQ_XHAT_HIGHER_L_ZERO), who ": the table form is the first block's (BT layout, XEQ_XHAT_HIGHER_L_ZERO)"); \
  } while (0)
