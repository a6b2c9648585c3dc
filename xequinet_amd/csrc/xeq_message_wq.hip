// Fused XPaiNN message kernels, "wave / quad" form (fp32; the default where the channel layout allows it).
// Reference dataflow: nn/xpainn.py:140-159; reverse pass for nn/basic.py:143-159.
//
// Arithmetic mapping (kept from round 1's wave / matrix-core form, xeq_message_wm.hip, retired in round 4): the filter
// phi_e = (W rho(d_e) + b) f(d_e) is a matrix-core tile D[edge][channel] (K = B + 1),
// a wave owns (range of nodes, 32 gate channels of one l), its two half-waves are two independent streams over
// contiguous CSR segments, and the sum over the edges of a node is a running sum in registers that is stored once.
//
// The WALK ORDER removes the per-row bookkeeping that bounded that form (19 vector
// instructions per MFMA, 244 VGPRs, a divergent first/last branch per row):
//
//   * every node's edge list is padded to a multiple of FOUR slots ("quads"; padding slots carry an all-zero record,
//     so their filter is exactly 0).  The four accumulator registers 4g .. 4g+3 of a lane are then the four rows of
//     ONE quad, and a quad belongs to ONE node: segment starts and ends can only fall between quads.  The rows of a
//     quad are plain FMAs into a quad sum; the segment logic (reset / residual / the node's only store) runs once
//     per quad on half-uniform flags, 4x less often and branch-free except for the store.
//   * the walk plan (xeq_message_wq_plan) is built once per graph, independent of the positions: per padded slot the
//     gathered node and the edge id, per quad the owner node and its first / last flags, stream boundaries on quads.
//     The per-edge records (xeq_edge_basis_wq) are written IN PADDED WALK ORDER, so a tile's A operand, its Y_lm and
//     its indices are sequential loads with no dependent index chain.
//   * what a whole quad shares comes from its owner: in the reverse pass the owner's rows (h, xhat) are per-quad
//     constants, so products with them are hoisted out of the rows (l = 0: 7 vector instructions per row).
//   * the per-edge sums over channels of the reverse pass (dL/dd, dL/dY_lm) use a register-halving DPP butterfly:
//     16 rows x 32 lanes reduce in 48 instead of 80 cross-lane adds, and leave as one 64-byte store per quantity.
//
// Three files, two objects with their own flags (csrc/build.py): this one holds the walk plan, the records, the weight packing and
// the forward kernel (LLVM's max-ILP machine scheduler: forward launch 201 against 212 us); xeq_message_wq_bwd.hip the reverse
// kernel and the edge gradients (default scheduler, which weighs register pressure: reverse launch 355 against 368 us);
// xeq_message_wq.h what both compile.  The variants that were measured and lost are no longer in the source: what each of them
// found is in profiles/HISTORY.md and profiles/r0*_small_experiments.txt.
#include "xeq_message_wq.h"

#include <hipcub/hipcub.hpp>

namespace xeq {

// ------------------------------------------------------------------------------------------------ walk plan
struct QuadCount {
  const int32_t* rowptr;
  int64_t n;
  // a node without an edge still gets ONE quad (four padding slots: zero records, gathering its own rows): it then takes the
  // ordinary path -- its running sums are exact zeros, its store writes s_out = s_in / zero gradients -- and the plan spreads such
  // nodes over the ranges by their quads.  (They used to be picked up range by range in a serial loop of one wave: the 400 padding
  // atoms of a capacity-sized batch sat behind the LAST range and cost 5 % of a step, 2 000 of them doubled it.)
  __host__ __device__ int32_t operator()(int64_t i) const {
    if (i >= n) return 0;
    const int32_t deg = rowptr[i + 1] - rowptr[i];
    return deg > 0 ? (deg + 3) >> 2 : 1;
  }
};
// qptr[0 .. n] = exclusive prefix sums of the quads per node, by one workgroup (xeq_common.h: wg_scan_lds)
__global__ void __launch_bounds__(SCAN_WG_THREADS) k_wq_quad_scan(const QuadCount op, int32_t* __restrict__ qptr) {
  extern __shared__ int32_t scan_lds[];
  const int32_t total = wg_scan_lds(op, op.n, scan_lds);
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < op.n; i += SCAN_WG_THREADS) qptr[i] = scan_lds[i];
  if (threadIdx.x == 0) qptr[op.n] = total;
}

// one thread per slot of the walk order: its padded position, the pads behind a segment's last slot, the quad records
__global__ void k_wq_fill(int64_t E, int64_t n_nodes, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                          const int64_t* __restrict__ owner, const int64_t* __restrict__ gather,
                          const int32_t* __restrict__ qptr, int32_t* __restrict__ pgath, int32_t* __restrict__ peid,
                          uint32_t* __restrict__ qinfo) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= E) {   // threads E .. E + N - 1: the lone quad of a node without an edge
    const int64_t n = s - E;
    if (n < n_nodes && rowptr[n] == rowptr[n + 1]) {
      const int64_t q0 = qptr[n];
      for (int i = 0; i < 4; ++i) {
        pgath[4 * q0 + i] = (int32_t)n;
        peid[4 * q0 + i] = -1;
      }
      qinfo[q0] = (uint32_t)n | WQ_FIRST | WQ_LAST;
    }
    return;
  }
  if (s >= rowptr[n_nodes]) return;   // E may be a capacity: the walk ends at rowptr[N] (device-side edge count)
  const int32_t eid = perm ? perm[s] : (int32_t)s;
  const int64_t n = owner[eid];
  const int32_t r0 = rowptr[n], deg = rowptr[n + 1] - r0, k = (int32_t)(s - r0), q0 = qptr[n], nq = (deg + 3) >> 2;
  const int64_t p = 4 * (int64_t)q0 + k;
  pgath[p] = (int32_t)gather[eid];
  peid[p] = eid;
  if (k == deg - 1)
    for (int64_t pp = p + 1; pp < 4 * (int64_t)(q0 + nq); ++pp) {   // pads: zero record, gather the owner's own rows
      pgath[pp] = (int32_t)n;
      peid[pp] = -1;
    }
  if ((k & 3) == 0) {
    const int32_t g = k >> 2;
    qinfo[q0 + g] = (uint32_t)n | (g == 0 ? WQ_FIRST : 0u) | (g == nq - 1 ? WQ_LAST : 0u);
  }
}

// sq[k] / sn[k]: first quad / node of stream k; boundaries sit on segment starts at about equal quad counts
__global__ void k_wq_streams(const int32_t* __restrict__ qptr, int64_t N, int n_ranges, int32_t* __restrict__ sq,
                             int32_t* __restrict__ sn) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > 2 * n_ranges) return;
  const int64_t Q = qptr[N];
  if (k == 2 * n_ranges) {
    sq[k] = (int32_t)Q;
    sn[k] = (int32_t)N;
    return;
  }
  const int64_t target = (int64_t)k * Q / (2 * n_ranges);
  int64_t lo = 0, hi = N;   // first n in [0, N] with qptr[n] >= target
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (qptr[mid] >= target) hi = mid;
    else lo = mid + 1;
  }
  sq[k] = qptr[lo];
  sn[k] = (int32_t)lo;
}

// win[2 s], win[2 s + 1]: first gathered node and number of rows of the WINDOW of step s = the WQ_WAVES consecutive
// ranges one workgroup walks together: every node its 2 WQ_WAVES streams gather from lies in [w0, w0 + rows).  One wave
// per step.  For batches of molecules the window is the few molecules the step touches.
// mult: the stream CLASS (wq_long_mult below): a stream of the class is `mult` consecutive streams of the table
__global__ void k_wq_windows(const int32_t* __restrict__ sq, const int32_t* __restrict__ pgath, int n_ranges, int n_steps, int mult,
                             int32_t* __restrict__ win) {
  const int step = blockIdx.x, lane = threadIdx.x;
  if (step >= n_steps) return;
  const int k0 = min(2 * WQ_WAVES * mult * step, 2 * n_ranges), k1 = min(k0 + 2 * WQ_WAVES * mult, 2 * n_ranges);
  const int64_t p0 = 4 * (int64_t)sq[k0], p1 = 4 * (int64_t)sq[k1];
  int lo = 0x7fffffff, hi = -1;
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const int g = pgath[p];
    lo = g < lo ? g : lo;
    hi = g > hi ? g : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (lane == 0) {
    win[2 * step] = hi >= 0 ? lo : 0;
    win[2 * step + 1] = hi >= 0 ? hi - lo + 1 : 0;
  }
}

// records in padded walk order (layout: WQ_REC above); val(k) = f rho_k, the bias column's multiplier is f; derivative record
// likewise.  Six threads per slot: two (one per k half) evaluate eight basis functions each and store their three bf16 packs,
// two the f32 tail, two the harmonics.
// one piece (grp: 0-1 bf16 packs of k half grp; 2-3 f32 tail of k half grp - 2; 4-5 harmonics) of the record of padded slot p, written
// through out / dout (the slot's record in the workgroup's LDS staging rows)
__device__ __forceinline__ void wq_record_piece(const float* __restrict__ vec, const int32_t* __restrict__ peid, int64_t p, int grp,
                                                const RadialSpec& rs, const float* __restrict__ p0, const float* __restrict__ p1,
                                                float* __restrict__ out, float* __restrict__ dout, int tailw, bool bftail) {
  const int yoff = WQ_TAIL + 2 * tailw;
  const int32_t e = peid[p];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (e < 0) {   // padding slot: an all-zero record (its filter is exactly 0)
    if (grp < 2) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<f32x4*>(out + 12 * grp + 4 * c) = zero;
        if (dout) *reinterpret_cast<f32x4*>(dout + 12 * grp + 4 * c) = zero;
      }
    } else if (grp < 4) {
      for (int c = 0; c < tailw; c += 4) {
        *reinterpret_cast<f32x4*>(out + WQ_TAIL + tailw * (grp - 2) + c) = zero;
        if (dout) *reinterpret_cast<f32x4*>(dout + WQ_TAIL + tailw * (grp - 2) + c) = zero;
      }
    } else {
      *reinterpret_cast<f32x4*>(out + yoff + 4 * (grp - 4)) = zero;
      if (dout) *reinterpret_cast<f32x4*>(dout + yoff + 4 * (grp - 4)) = zero;
    }
    return;
  }
  const float rc = (float)rs.cutoff;
  const EdgeGeom<float> g = edge_geom<float>(vec[3 * (int64_t)e], vec[3 * (int64_t)e + 1], vec[3 * (int64_t)e + 2]);
  const int B = rs.num_basis;
  if (grp >= 4) {
    float y1[3], y2[5];
    sph_harm_l12<float>(g, y1, y2);
    const f32x4 v = grp == 4 ? f32x4{y1[0], y1[1], y1[2], y2[0]} : f32x4{y2[1], y2[2], y2[3], y2[4]};
    *reinterpret_cast<f32x4*>(out + yoff + 4 * (grp - 4)) = v;
    if (dout) *reinterpret_cast<f32x4*>(dout + yoff + 4 * (grp - 4)) = v;   // the reverse kernel reads Y next to the derivatives (one record
    return;                                                                  // stream less per row load; measured: no change in traffic or
                                                                             // time -- the l > 0 units need the value record anyway, for the
                                                                             // gate_edge filter in dL/dY)
  }
  float f, df;
  envelope<float>(rs.cutoff_kind, g.d, rc, f, df);
  auto value = [&](int k, float& val, float& dval) {   // k >= 0: basis function k; -1: the bias column; -2: nothing
    val = dval = 0.f;
    if (k >= 0 && k < B) {
      float rho, drho;
      radial<float>(rs.rbf_kind, g.d, rc, p0[k], p1 ? p1[k] : 0.f, rho, drho, k, B);
      val = f * rho;
      dval = df * rho + f * drho;
    } else if (k == -1) {
      val = f;
      dval = df;
    }
  };
  if (grp < 2) {
    const int kh = grp;
    uint32_t w[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, dw[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      float val, dval;
      value(8 * kh + jj < B ? 8 * kh + jj : -2, val, dval);
      uint32_t a3[3], d3[3];
      wq_split3(val, a3[0], a3[1], a3[2]);
      wq_split3(dval, d3[0], d3[1], d3[2]);
#pragma unroll
      for (int sp = 0; sp < 3; ++sp) {
        w[sp][jj >> 1] |= a3[sp] << (16 * (jj & 1));
        dw[sp][jj >> 1] |= d3[sp] << (16 * (jj & 1));
      }
    }
#pragma unroll
    for (int sp = 0; sp < 3; ++sp) {
      *reinterpret_cast<f32x4*>(out + 12 * kh + 4 * sp) =
          f32x4{__uint_as_float(w[sp][0]), __uint_as_float(w[sp][1]), __uint_as_float(w[sp][2]), __uint_as_float(w[sp][3])};
      if (dout)
        *reinterpret_cast<f32x4*>(dout + 12 * kh + 4 * sp) =
            f32x4{__uint_as_float(dw[sp][0]), __uint_as_float(dw[sp][1]), __uint_as_float(dw[sp][2]), __uint_as_float(dw[sp][3])};
    }
  } else if (bftail) {   // slots 8 kh .. 8 kh + 7 of [hi_0..4 | mid_0..4 | lo_0..4 | 0]: the three bf16 parts of the five tail values
    const int kh = grp - 2;
    uint32_t a3[5][3], d3[5][3];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float val, dval;
      value(wq_tail_k(q, B), val, dval);
      wq_split3(val, a3[q][0], a3[q][1], a3[q][2]);
      wq_split3(dval, d3[q][0], d3[q][1], d3[q][2]);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u}, dw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int sl0 = jj, sl1 = 8 + jj;   // (both k halves unrolled, one selected: the slot arithmetic stays compile-time)
      const uint32_t v0 = sl0 < 15 ? a3[sl0 % 5][sl0 / 5] : 0u, v1 = sl1 < 15 ? a3[sl1 % 5][sl1 / 5] : 0u;
      const uint32_t e0 = sl0 < 15 ? d3[sl0 % 5][sl0 / 5] : 0u, e1 = sl1 < 15 ? d3[sl1 % 5][sl1 / 5] : 0u;
      w[jj >> 1] |= (kh ? v1 : v0) << (16 * (jj & 1));
      dw[jj >> 1] |= (kh ? e1 : e0) << (16 * (jj & 1));
    }
    *reinterpret_cast<f32x4*>(out + WQ_TAIL + 4 * kh) = f32x4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
    if (dout)
      *reinterpret_cast<f32x4*>(dout + WQ_TAIL + 4 * kh) = f32x4{__uint_as_float(dw[0]), __uint_as_float(dw[1]), __uint_as_float(dw[2]), __uint_as_float(dw[3])};
  } else {
    const int kh = grp - 2;
    for (int c0 = 0; c0 < tailw; c0 += 4) {   // tail value s of this k half: position q = 2 s + kh
      f32x4 v, dv;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float val, dval;
        value(wq_tail_k(2 * (c0 + c) + kh, B), val, dval);
        v[c] = val;
        dv[c] = dval;
      }
      *reinterpret_cast<f32x4*>(out + WQ_TAIL + tailw * kh + c0) = v;
      if (dout) *reinterpret_cast<f32x4*>(dout + WQ_TAIL + tailw * kh + c0) = dv;
    }
  }
}


// A workgroup writes the records of WQ_REC_SLOTS consecutive padded slots: waves 0 / 1 / 2 compute the bf16 packs / the f32 tails / the
// harmonics of all of them (one KIND of piece per wave: with the six pieces of a slot on six neighbouring lanes every wave ran all three
// branches one after the other at a third of its lanes) into LDS rows, then all 256 threads store the rows with whole 16-byte lanes
// (the pieces are 16-48 bytes at a stride of 160: stored directly they kept the kernel at 2.6 TB/s of writes).  48.5 -> 42 us with the
// wave-uniform kinds alone; the same values bit for bit.
constexpr int WQ_REC_SLOTS = 32;
struct WqTableIndex {
  const void* z;            // [N] atomic numbers = rows of the element table (NULL: no table rows wanted)
  int z_is_int64;
  int64_t rows;
  const int32_t* pgath;     // the plan's gathered node per slot / owner per quad
  const uint32_t* qinfo;
  int32_t* ptab;            // [P] out
  int32_t* qtab;            // [P / 4] out
  // (a number outside the table reads row 0, the table's all-zero padding row, as xeq_first_block_front does)
  __device__ __forceinline__ int32_t row(int32_t node) const {
    const int64_t v = z_is_int64 ? ((const int64_t*)z)[node] : (int64_t)((const int32_t*)z)[node];
    return v >= 0 && v < rows ? (int32_t)v : 0;
  }
};
__global__ void __launch_bounds__(256) k_wq_records(const float* __restrict__ vec, const int32_t* __restrict__ peid,
                             const int32_t* __restrict__ qptr, int64_t N, int64_t pcap, RadialSpec rs,
                             const float* __restrict__ p0, const float* __restrict__ p1, float* __restrict__ rec,
                             float* __restrict__ drec, int recf, int tailw, int bftail, const WqTableIndex ti) {
  __shared__ __attribute__((aligned(16))) float stage[2][WQ_REC_SLOTS * 48];
  const int64_t limit = min(pcap, 4 * (int64_t)qptr[N]);
  const int64_t first = (int64_t)blockIdx.x * WQ_REC_SLOTS;
  if (first >= limit) return;                                   // uniform
  const int t = threadIdx.x, kind = t >> 6, r = t & 63, slot = r >> 1;
  const int64_t p = first + slot;
  if (kind < 3 && p < limit)
    wq_record_piece(vec, peid, p, 2 * kind + (r & 1), rs, p0, p1, stage[0] + slot * recf, drec ? stage[1] + slot * recf : nullptr, tailw, bftail != 0);
  // the fourth wave has no piece to compute: it writes the element-table rows of the first block's table form (xeq_edge_basis_wq_table),
  // per padded slot the row of the gathered node and per quad the row of its owner, so that the message kernels find them by sequential
  // loads next to pgath / qinfo instead of through the node id
  if (kind == 3 && ti.z) {
    if (r < WQ_REC_SLOTS) {
      if (first + r < limit) ti.ptab[first + r] = ti.row(ti.pgath[first + r]);
    } else if (r < WQ_REC_SLOTS + WQ_REC_SLOTS / 4) {
      const int64_t q = first / 4 + (r - WQ_REC_SLOTS);
      if (4 * q < limit) ti.qtab[q] = ti.row((int32_t)(ti.qinfo[q] & WQ_OWNER));
    }
  }
  __syncthreads();
  const int n4 = (int)min((int64_t)WQ_REC_SLOTS, limit - first) * recf / 4;
  const f32x4* s0 = reinterpret_cast<const f32x4*>(stage[0]);
  const f32x4* s1 = reinterpret_cast<const f32x4*>(stage[1]);
  f32x4* g0 = reinterpret_cast<f32x4*>(rec + first * recf);
  f32x4* g1 = drec ? reinterpret_cast<f32x4*>(drec + first * recf) : nullptr;
  for (int i = t; i < n4; i += 256) {
    g0[i] = s0[i];
    if (g1) g1[i] = s1[i];
  }
}

// ------------------------------------------------------------------------------------------------ forward
// scheduling fence between the passes of a tile (dev switch: -D'XEQ_WQ_SB()=' compiles them out)
#ifndef XEQ_WQ_SB
#define XEQ_WQ_SB() __builtin_amdgcn_sched_barrier(0)
#endif
// fence between the phases of a forward tile (dev switch: -D'XEQ_WQ_FSB()=' lets the compiler interleave them).  FENCED (template
// parameter of the forward body): the first-block kernel runs WITHOUT the fences since round 6 -- its launch 113.6 -> 109.7 us, the general
// kernel's the same with and without (profiles/r06_small_experiments.txt item 12)
#ifndef XEQ_WQ_FSB
#define XEQ_WQ_FSB() do { if constexpr (FENCED) XEQ_WQ_SB(); } while (0)
#endif
#ifndef XEQ_WQ_FWD_WPE
#define XEQ_WQ_FWD_WPE 2
#endif

// window of the forward pass: per row the unit's pieces of h (gate_state | gate_edge | scalar message for l = 0) and of
// xhat (NM pieces: component m in BT layout; the contiguous run of 32 NM floats in e3nn layout)
// XZ (l > 0 only): xhat is zero on the unit's columns (first block of the model), so only the gate_edge piece is staged
template <int NM, bool XZ>
__device__ __forceinline__ void wq_stage_fwd(const WqArgs& a, const WqUnit& un, const WqCols& wc, const float* __restrict__ h,
                                             const float* __restrict__ xhat_, int w0, int nrows, float* win) {
  constexpr int NH = NM == 1 ? 3 : 2, NSL = NH + NM;
  if constexpr (XZ && NM > 1) {
    const int total = nrows * 8;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int row = idx >> 3, chunk = idx & 7;
      *reinterpret_cast<f32x4*>(win + (row * NSL + 1) * 32 + 4 * chunk) =
          *reinterpret_cast<const f32x4*>(h + (int64_t)(w0 + row) * a.H + a.C + un.u0 + 4 * chunk);
    }
    return;
  }
  const int total = nrows * NSL * 8;   // 16-byte chunks
  const int64_t xnode = wc.xnode_b / 4, xcomp = a.xl == 0 ? 32 : wc.xcomp_b / 4;
  constexpr int UN = 8;                // loads in flight per thread before the first LDS store
  const int nthr = blockDim.x;
  for (int base = threadIdx.x; base < total; base += UN * nthr) {
    f32x4 v[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int idx = base + k * nthr;
      const int piece = idx >> 3, chunk = idx & 7;
      const int row = piece / NSL, sl = piece - row * NSL;
      const int64_t n = w0 + (idx < total ? row : 0);
      const float* src = sl < NH ? h + n * a.H + (sl == 0 ? un.u0 : (sl == 1 ? a.C + un.u0 : 2 * a.C + 32 * un.cb))
                                 : xhat_ + wc.x_base + n * xnode + (sl - NH) * xcomp;
      v[k] = *reinterpret_cast<const f32x4*>(src + 4 * chunk);   // a slot beyond the window re-reads row w0: in bounds
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int idx = base + k * nthr;
      if (idx < total) *reinterpret_cast<f32x4*>(win + (idx >> 3) * 32 + 4 * (idx & 7)) = v[k];
    }
  }
}

// Table form of the first block (TAB): behind the embedding h and the 0e block of xhat are functions of the element, so what the
// forward pass gathers per edge is one of the T rows of the element table (h_table [T, H], xhat0_table [T, F]: what
// xeq_first_block_front gathers from).  The workgroup copies its unit's columns of the WHOLE table into the window's LDS once, behind
// its weights, in the window's row layout -- l = 0: [gate_state | gate_edge | scalar message | xhat_0] (512 bytes per row); l > 0, where
// xhat is zero: [gate_edge] (128 bytes) -- and every step reads it as a window that starts at row 0 and is indexed by the slot's TABLE
// row (a.pgath points at xeq_edge_basis_wq_table's per-slot rows): no window staging, no barrier per step, and the same LDS reads
// feeding the same arithmetic as the window form.
constexpr int wq_tab_row_bytes(int NM) { return NM == 1 ? 512 : 128; }
template <int NM>
__device__ __forceinline__ void wq_stage_table_fwd(const WqArgs& a, const WqUnit& un, const float* __restrict__ h_tab,
                                                   const float* __restrict__ x0_tab, float* win) {
  constexpr int NP = NM == 1 ? 4 : 1;   // 128-byte pieces per row
  const int total = a.tab_rows * NP * 8;   // 16-byte chunks
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int piece = idx >> 3, chunk = idx & 7;
    const int row = piece / NP, sl = piece - row * NP;
    const float* src = NM > 1 ? h_tab + (int64_t)row * a.H + a.C + un.u0
                              : (sl < 3 ? h_tab + (int64_t)row * a.H + (sl == 0 ? un.u0 : (sl == 1 ? a.C + un.u0 : 2 * a.C + 32 * un.cb))
                                        : x0_tab + (int64_t)row * a.F + un.u0);
    *reinterpret_cast<f32x4*>(win + piece * 32 + 4 * chunk) = *reinterpret_cast<const f32x4*>(src + 4 * chunk);
  }
}

//   x_c += xhat[n] (h_state[n] phi_state) + Y (h_edge[n] phi_edge);   s_c += h_msg[n] phi_msg   (l = 0)
// WIN: the gathered rows of this step are in the LDS window (first node w0); otherwise they are read from global memory
// TAB (with WIN): the "window" is the element table (above)
template <int NM, int KS, bool WIN, bool XZ, bool FENCED, bool TAB = false>
__device__ __forceinline__ void wq_fwd_body(const WqArgs& a, int range, const WqUnit un, const WqCols& wc,
                                            const float* __restrict__ rec, const float* __restrict__ h,
                                            const float* __restrict__ xhat_, const float* __restrict__ s_in,
                                            const float* __restrict__ x_in, const float* wl, float* __restrict__ s_out,
                                            float* __restrict__ x_out, int* tbl, const float* win, int w0,
                                            unsigned long long* st_, unsigned long long& last_) {
  constexpr bool HAS_S = NM == 1;
  constexpr bool NO_STATE = XZ && NM > 1;   // xhat = 0 on these columns: the gate_state term vanishes with its filter and gathers
  constexpr int YOFF = NM == 3 ? 0 : 3;
  static_assert(!TAB || (WIN && (XZ || NM == 1)), "the table form is a window form of the first block");
  constexpr int NH = NM == 1 ? 3 : 2, ROWB = TAB ? wq_tab_row_bytes(NM) : (NH + NM) * 128;
  constexpr uint32_t HE_OFF = TAB && NM > 1 ? 0u : 128u;   // the gate_edge piece inside a row
  const int lane = threadIdx.x & 63, j = lane & 31, hh = lane >> 5;
  const uint32_t row_s = 4u * (uint32_t)a.F, row_x = 4u * (uint32_t)a.D;
  wq_for_isolated(a, range, lane, [&](int m) {   // s_out = s_in, x_out = x_in on the unit's columns
    if (hh == 0) {
      if constexpr (HAS_S) wq_st(s_out, (uint32_t)m * row_s + wc.b_s, wq_ld(s_in, (uint32_t)m * row_s + wc.b_s));
#pragma unroll
      for (int mm = 0; mm < NM; ++mm)
        wq_st(x_out, (uint32_t)m * row_x + wc.b_xe + 4u * mm, wq_ld(x_in, (uint32_t)m * row_x + wc.b_xe + 4u * mm));
    }
  });
  const WqStreams st = wq_streams(a, range, un.l == 0 ? a.mlong : 1);
  if (st.ntiles == 0) return;
  const float* __restrict__ h_e = h + a.C;
  const float* __restrict__ h_m = h + (2 * a.C + 32 * un.cb - un.u0);
  const float* xhat_m[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) xhat_m[m] = xhat_ + wc.x_base + (int64_t)m * (wc.xcomp_b / 4);
  const uint32_t stride0 = WIN ? (uint32_t)ROWB : 4u * (uint32_t)a.H, stride1 = WIN ? 0u : wc.xnode_b;
  const uint32_t gbase = WIN ? (uint32_t)w0 : 0u;
  // window mode: byte offset of this lane's element of component m inside a row's xhat pieces
  uint32_t lxm[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) lxm[m] = (uint32_t)(NH * 128) + (a.xl == 0 ? 4u * (uint32_t)(j * NM + m) : (uint32_t)(128 * m + 4 * j));
  const float* Ws = wl;
  const float* We = wl + WQ_WK<KS>;
  const float* Wm = wl + 2 * WQ_WK<KS>;

  float acc_s = 0.f, acc_x[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) acc_x[m] = 0.f;

  using Row = WqRow<KS, 1, (NM > 1)>;
  Row row;
  wq_row<KS, 1, (NM > 1)>(a, st, lane, 0, rec, nullptr, row, (int)gbase);
  wq_publish<KS, 1, (NM > 1)>(lane, row, stride0, stride1, tbl, gbase);
  __builtin_amdgcn_wave_barrier();

  // A tile runs as four phases with every load of the tile issued up front (two waves per SIMD: 256 registers), so a
  // wave has ONE dependent wait per phase instead of one per quad (measured before: 52 % of a wave's cycles in
  // s_waitcnt, 28 % in issue stalls behind its own MFMA chain, 12 k cycles per tile):
  //   A  table entries of all 16 rows, the four owners' residual rows, the next tile's record (global, long latency)
  //   B  the gathered rows of all 16 rows (LDS window, or global memory)
  //   C  the MFMA chains of the filter
  //   D  row arithmetic, quad by quad; the finished nodes' stores
  // (A finished node's sums stored at the top of the NEXT tile, as the reverse kernel does with its per-edge partials, measured 278 -> 284 us
  // per forward pair: profiles/r06_small_experiments.txt item 12 c.)
  for (int t = 0; t < st.ntiles; ++t) {
    const int* tb = tbl + (t & 1) * T_SIZE;
    int* tnext = tbl + ((t + 1) & 1) * T_SIZE;
    const WqR<KS> R = row.R[0];
    WQ_STAMP(4);   // waiting for the tile's record
    // ---- phase A
    uint32_t g0[16], g1[WIN ? 1 : 16], ob[4], os[4];
    int keep[4], last[4];
    float res_x[4][NM], res_s[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t t0[4];
      wq_tread4<uint32_t>(tb, T_G0 + 16 * hh + 4 * g, t0);
#pragma unroll
      for (int r = 0; r < 4; ++r) g0[4 * g + r] = t0[r];
      if constexpr (!WIN) {
        uint32_t t1[4];
        wq_tread4<uint32_t>(tb, T_G1 + 16 * hh + 4 * g, t1);
#pragma unroll
        for (int r = 0; r < 4; ++r) g1[4 * g + r] = t1[r];
      }
      const uint32_t own = (uint32_t)tb[T_QOWN + 4 * hh + g];
      keep[g] = tb[T_QKEEP + 4 * hh + g];
      last[g] = tb[T_QLAST + 4 * hh + g];
      ob[g] = own * row_x + wc.b_xe;
      os[g] = own * row_s + wc.b_s;
#pragma unroll
      for (int m = 0; m < NM; ++m) res_x[g][m] = wq_ld(x_in, ob[g] + 4u * m);   // the owner's residual row, read per quad
      res_s[g] = HAS_S ? wq_ld(s_in, os[g]) : 0.f;
    }
    XEQ_WQ_FSB();   // the residual rows are requested IN FRONT of the next tile's record: memory returns in order, and the rows are consumed
                    // in this tile (waiting for them must not wait for the record prefetch behind them)
    wq_row<KS, 1, (NM > 1)>(a, st, lane, t + 1, rec, nullptr, row, (int)gbase);   // next tile's record flies under this tile
    XEQ_WQ_FSB();
    WQ_STAMP(5);   // phase A issued
    // ---- phases B, C, D; l = 2 gathers and consumes its rows in two halves of 8 (register budget)
    constexpr int GR = NM == 5 ? 8 : 16;
    f32x16 ds, de, dm;
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += GR) {
      float hs[GR], he[GR], hm[HAS_S ? GR : 1], xv[GR][NM];
#pragma unroll
      for (int u = 0; u < GR; ++u) {
        const int v = r0 + u;
        if constexpr (WIN) {
          const uint32_t oh = g0[v] + 4u * (uint32_t)j;
          if constexpr (!NO_STATE) hs[u] = wq_lds(win, oh);
          he[u] = wq_lds(win, oh + HE_OFF);
          if constexpr (HAS_S) hm[u] = wq_lds(win, oh + 256u);
          if constexpr (!NO_STATE) {
#pragma unroll
            for (int m = 0; m < NM; ++m) xv[u][m] = wq_lds(win, g0[v] + lxm[m]);
          }
        } else {
          const uint32_t oh = g0[v] + wc.b_hs, ox = g1[v] + wc.b_x;
          if constexpr (!NO_STATE) hs[u] = wq_ld(h, oh);
          he[u] = wq_ld(h_e, oh);
          if constexpr (HAS_S) hm[u] = wq_ld(h_m, oh);
          if constexpr (!NO_STATE) {
#pragma unroll
            for (int m = 0; m < NM; ++m) xv[u][m] = wq_ld(xhat_m[m], ox);
          }
        }
      }
      XEQ_WQ_FSB();
      WQ_STAMP(6);   // phase B issued
      if (r0 == 0) {   // ---- phase C
        de = wq_filter<KS>(R, We, lane);
        ds = de;
        if constexpr (!NO_STATE) ds = wq_filter<KS>(R, Ws, lane);
        dm = ds;
        if constexpr (HAS_S) dm = wq_filter<KS>(R, Wm, lane);
        XEQ_WQ_FSB();
        WQ_STAMP(7);   // MFMAs issued
      }
      // ---- phase D
#pragma unroll
      for (int g = r0 / 4; g < (r0 + GR) / 4; ++g) {
        float Y[NM][4];
        if constexpr (NM > 1) {
#pragma unroll
          for (int m = 0; m < NM; ++m) wq_tread4<float>(tb, T_Y + 32 * (YOFF + m) + 16 * hh + 4 * g, Y[m]);
        }
        float xq[NM], sq = 0.f;
#pragma unroll
        for (int m = 0; m < NM; ++m) xq[m] = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = 4 * g + r, u = v - r0;
          // explicit fma chains (this file is built with -ffp-contract=off): the window and the global instantiation of
          // this body must round alike, or a node's result would depend on which one its step took
          const float ge = he[u] * de[v];
          if constexpr (NO_STATE) {   // fma(0, gs, c) = c: the same bits as the general form on xhat = 0
#pragma unroll
            for (int m = 0; m < NM; ++m) xq[m] = __builtin_fmaf(Y[m][r], ge, xq[m]);
          } else {
            const float gs = hs[u] * ds[v];
#pragma unroll
            for (int m = 0; m < NM; ++m) xq[m] = __builtin_fmaf(xv[u][m], gs, NM > 1 ? __builtin_fmaf(Y[m][r], ge, xq[m]) : xq[m] + ge);
          }
          if constexpr (HAS_S) sq = __builtin_fmaf(hm[u], dm[v], sq);
        }
        // A node's running sums START from its residual row (round 6; up to round 5 the residual was added at the store).  The residual
        // rows are requested at the tile top; used only inside `if (last)` their loads were SUNK into that branch by the compiler -- a
        // global round trip behind an s_waitcnt vmcnt(0) per finished node, which also drained the next tile's record prefetch.  Consumed
        // here by a select they stay where they are requested.  (Order of a node's additions: ((res + q_0) + q_1) + ... in any batch.)
#pragma unroll
        for (int m = 0; m < NM; ++m) acc_x[m] = (keep[g] ? acc_x[m] : res_x[g][m]) + xq[m];
        if constexpr (HAS_S) acc_s = (keep[g] ? acc_s : res_s[g]) + sq;
        if (last[g]) {   // the node's only store
#pragma unroll
          for (int m = 0; m < NM; ++m) wq_st(x_out, ob[g] + 4u * m, acc_x[m]);
          if constexpr (HAS_S) wq_st(s_out, os[g], acc_s);
        }
      }
      if constexpr (GR < 16) XEQ_WQ_FSB();
      WQ_STAMP(8);   // phase D: row arithmetic and stores
    }
    wq_publish<KS, 1, (NM > 1)>(lane, row, stride0, stride1, tnext, gbase);
    __builtin_amdgcn_wave_barrier();
    WQ_STAMP(9);   // next table published
  }
}


// one role of the forward kernel: the workgroup's steps, each with its window staged first when it fits
template <int NM, int KS, bool XZ, bool FENCED, bool TAB = false>
__device__ __forceinline__ void wq_fwd_role(const WqArgs& a, int s_beg, int s_end, const WqUnit un, const float* __restrict__ rec,
                                            const float* __restrict__ h, const float* __restrict__ xhat,
                                            const float* __restrict__ s_in, const float* __restrict__ x_in, const float* wl,
                                            float* __restrict__ s_out, float* __restrict__ x_out, int* tbl, float* win) {
  constexpr int NH = NM == 1 ? 3 : 2, ROWB = (NH + NM) * 128;
  const WqCols wc = wq_cols<NM>(a, un, threadIdx.x & 31);
  unsigned long long st_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = 0;
#ifdef XEQ_WQ_STAMPS
  last_ = __builtin_amdgcn_s_memtime();
#endif
  // the workgroup's chunk [s_beg, s_end) counts UNITS of a.mlong short steps = one long step: the steps of this unit's class in it
  const WqClass cl = wq_class(a, un.l);
  const int c_beg = cl.m == a.mlong ? s_beg : s_beg * a.mlong, c_end = min(cl.m == a.mlong ? s_end : s_end * a.mlong, cl.n_steps);
  if constexpr (TAB) {   // the table is staged (kernel top): the waves walk their ranges of the chunk's steps without meeting again
    for (int step = c_beg; step < c_end; ++step) {
      const int range = step * WQ_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      if (range < cl.n_ranges) wq_fwd_body<NM, KS, true, XZ, FENCED, true>(a, range, un, wc, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win, 0, st_, last_);
    }
    return;
  }
  for (int step = c_beg; step < c_end; ++step) {
    const int w0 = cl.win[2 * step], nrows = cl.win[2 * step + 1];
    const bool use_win = nrows > 0 && nrows * ROWB <= WQ_WIN_FLOATS * 4;   // workgroup-uniform
    WQ_STAMP(0);   // step head
    if (use_win) wq_stage_fwd<NM, XZ>(a, un, wc, h, xhat, w0, nrows, win);
    WQ_STAMP(1);   // window staged
    __syncthreads();
    WQ_STAMP(2);   // barrier behind the staging
    const int range = step * WQ_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: the stream bounds become scalar loads)
    if (range < cl.n_ranges) {
      if (use_win) wq_fwd_body<NM, KS, true, XZ, FENCED>(a, range, un, wc, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win, w0, st_, last_);
      else wq_fwd_body<NM, KS, false, XZ, FENCED>(a, range, un, wc, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win, 0, st_, last_);
    }
    WQ_STAMP(3);   // body prologue (isolated nodes, first record) -- what the tile stamps did not take
    __syncthreads();   // the window and the tile tables are rewritten by the next step
    WQ_STAMP(10);  // barrier behind the step
  }
#ifdef XEQ_WQ_STAMPS
  if (NM == 1 && (threadIdx.x & 63) == 0) {
    for (int i = 0; i < 11; ++i) atomicAdd(&g_wq_stamps[i], st_[i]);
    atomicAdd(&g_wq_stamps[15], 1ull);
  }
#endif
}

// The units' rbf_lin rows in the kernels' LDS layout, once per weight version (xeq_message_wq_pack_weights): a workgroup per unit runs
// the very staging code of the kernels into global memory.  Why: that staging reads w[row B + k] with one ROW PER LANE -- 64 cache
// lines per wave instruction, 24 such instructions per workgroup -- and sits between every two workgroups of a CU slot: ~11 us of a
// 160-280 us launch (timing-only variant with a coalesced copy: forward 181 -> 170 us, reverse 296 -> 285 us).
template <int KS>
__global__ void __launch_bounds__(256) k_wq_pack_weights(WqArgs a, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ out) {
  const WqUnit un = wq_unit(a, (int)blockIdx.x);
  float* dst = out + (size_t)blockIdx.x * (3 * WQ_WK<KS>);
  if (un.l != 0)   // (two kinds only: the third block of the unit's slot reads as zeros)
    for (int idx = threadIdx.x; idx < WQ_WK<KS>; idx += blockDim.x) dst[2 * WQ_WK<KS> + idx] = 0.f;
  wq_stage_weights<KS>(a, un, w, b, dst);
}

// XZ: xhat is zero on every l > 0 column (the model's first message block: XEmbedding hands over x = 0, and the
// equivariant layer norm of zero is zero there); the l = 0 role is the general one
// TAB (with XZ): h / xhat point at the element table's rows and a.pgath at the slots' table rows (table form, above)
template <int KS, bool XZ, bool TAB = false>
__global__ void __launch_bounds__(64 * WQ_WAVES) __attribute__((amdgpu_waves_per_eu(XEQ_WQ_FWD_WPE)))
k_message_fwd_wq(WqArgs a, const float* __restrict__ rec, const float* __restrict__ h, const float* __restrict__ xhat,
                 const float* __restrict__ s_in, const float* __restrict__ x_in, const float* __restrict__ w_rbf,
                 const float* __restrict__ b_rbf, float* __restrict__ s_out, float* __restrict__ x_out) {
  __shared__ __attribute__((aligned(16))) float win[WQ_WIN_FLOATS];
  __shared__ __attribute__((aligned(16))) int tbl_all[WQ_WAVES][2 * T_SIZE];
  __shared__ __attribute__((aligned(16))) float wl[3 * WQ_WK<KS>];
  int s_beg, s_end, unit;
  wq_decode(a, a.nu[0] + a.nu[1] + a.nu[2], s_beg, s_end, unit);
  if (s_beg >= s_end) return;   // padding block of the grid / empty chunk of a short region (workgroup-uniform)
  const WqUnit un = wq_unit(a, unit);
  wq_stage_weights<KS>(a, un, w_rbf, b_rbf, wl);
  if constexpr (TAB) {
    static_assert(XZ, "the table form is a first-block form");
    if (un.l == 0) wq_stage_table_fwd<1>(a, un, h, xhat, win);
    else wq_stage_table_fwd<3>(a, un, h, xhat, win);   // (l = 1 and l = 2 alike: the unit's gate_edge columns)
  }
  __syncthreads();
  int* tbl = tbl_all[threadIdx.x >> 6];
#ifdef XEQ_WQ_ROLE_TIME_FWD   // development: where and when every workgroup of the production body ran
  unsigned long long rr0_;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rr0_)::"memory");
#endif
  if (un.l == 0) wq_fwd_role<1, KS, false, !XZ, TAB>(a, s_beg, s_end, un, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win);
  else if (un.l == 1) wq_fwd_role<3, KS, XZ, !XZ, TAB>(a, s_beg, s_end, un, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win);
  else wq_fwd_role<5, KS, XZ, !XZ, TAB>(a, s_beg, s_end, un, rec, h, xhat, s_in, x_in, wl, s_out, x_out, tbl, win);
#ifdef XEQ_WQ_ROLE_TIME_FWD
  if (threadIdx.x == 0 && blockIdx.x < 8192) {
    unsigned long long rr1_;
    unsigned hw, xcc;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_getreg_b32 %1, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %2, hwreg(HW_REG_XCC_ID)\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(rr1_), "=s"(hw), "=s"(xcc)::"memory");
    g_wq_wg[4 * blockIdx.x + 0] = hw | ((unsigned long long)un.l << 32);
    g_wq_wg[4 * blockIdx.x + 1] = xcc;
    g_wq_wg[4 * blockIdx.x + 2] = rr0_;
    g_wq_wg[4 * blockIdx.x + 3] = rr1_;
  }
#endif
}


}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_message_wq_table_max_rows(void) { return WQ_TAB_MAX_ROWS; }

int xeq_message_wq_supported(int num_basis, int node_dim, const int32_t mul[3]) { return wq_supported(num_basis, node_dim, mul) ? 1 : 0; }

int xeq_message_wq_fits(int64_t n_nodes, int64_t n_edges, int num_basis, int node_dim, const int32_t mul[3]) {
  return wq_supported(num_basis, node_dim, mul) && n_nodes < (1ll << 30) && wq_fits(n_nodes, n_edges, node_dim, mul) ? 1 : 0;
}

int64_t xeq_message_wq_pcap(int64_t n_nodes, int64_t n_edges) { return wq_pcap(n_nodes, n_edges); }

int xeq_message_wq_waves(void) { return WQ_WAVES; }

int xeq_message_wq_record_floats(void) { return wq_recf(4); }   /* up to 23 basis functions */
int xeq_message_wq_record_floats_for(int num_basis) { return wq_recf(wq_ks(num_basis)); }

int64_t xeq_message_wq_plan_workspace(int64_t n_nodes) {
  size_t temp = 0;
  QuadCount op{nullptr, n_nodes};
  hipcub::CountingInputIterator<int64_t> cnt(0);
  hipcub::TransformInputIterator<int32_t, QuadCount, hipcub::CountingInputIterator<int64_t>> it(cnt, op);
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, temp, it, (int32_t*)nullptr, (int)(n_nodes + 1)) != hipSuccess) return -1;
  return (int64_t)temp + 256;
}

int xeq_message_wq_plan(const int32_t* rowptr, const int32_t* perm, const int64_t* owner, const int64_t* gather,
                        int64_t n_nodes, int64_t n_edges, int n_ranges, void* workspace, int64_t workspace_bytes,
                        int32_t* qptr, int32_t* pgath, int32_t* peid, int32_t* qinfo, int32_t* sq, int32_t* sn, int32_t* win,
                        void* stream) {
  XEQ_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_ranges >= 1 && n_nodes < (1ll << 30) && n_edges < (1ll << 31), "xeq_message_wq_plan: bad sizes");
  const int64_t need = xeq_message_wq_plan_workspace(n_nodes);
  XEQ_CHECK_ARG(need >= 0 && workspace_bytes >= need, "xeq_message_wq_plan: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
  QuadCount op{rowptr, n_nodes};
  if (n_nodes <= SCAN_WG_MAX_ITEMS) {   // one workgroup, one launch (the grid-wide scan is two)
    static const bool attr_ok = hipFuncSetAttribute((const void*)k_wq_quad_scan, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)wg_scan_lds_bytes(SCAN_WG_MAX_ITEMS)) == hipSuccess;
    XEQ_CHECK_ARG(attr_ok, "xeq_message_wq_plan: cannot reserve LDS for the quad scan");
    hipLaunchKernelGGL(k_wq_quad_scan, dim3(1), dim3(SCAN_WG_THREADS), wg_scan_lds_bytes(n_nodes), (hipStream_t)stream, op, qptr);
    XEQ_CHECK_LAUNCH("xeq_message_wq_plan (quad scan)");
  } else {
    hipcub::CountingInputIterator<int64_t> cnt(0);
    hipcub::TransformInputIterator<int32_t, QuadCount, hipcub::CountingInputIterator<int64_t>> it(cnt, op);
    size_t temp = (size_t)workspace_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(workspace, temp, it, qptr, (int)(n_nodes + 1), (hipStream_t)stream) != hipSuccess) {
      xeq::set_error("xeq_message_wq_plan: scan failed");
      return XEQ_ERR_LAUNCH;
    }
  }
  if (n_edges + n_nodes > 0) {
    hipLaunchKernelGGL(k_wq_fill, dim3((unsigned)((n_edges + n_nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_edges, n_nodes,
                       rowptr, perm, owner, gather, (const int32_t*)qptr, pgath, peid, (uint32_t*)qinfo);
    XEQ_CHECK_LAUNCH("xeq_message_wq_plan (fill)");
  }
  const int n = 2 * n_ranges + 1;
  hipLaunchKernelGGL(k_wq_streams, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int32_t*)qptr,
                     n_nodes, n_ranges, sq, sn);
  XEQ_CHECK_LAUNCH("xeq_message_wq_plan (streams)");
  const int n_steps = wq_class_steps(n_ranges, 1);
  hipLaunchKernelGGL(k_wq_windows, dim3((unsigned)n_steps), dim3(64), 0, (hipStream_t)stream, (const int32_t*)sq,
                     (const int32_t*)pgath, n_ranges, n_steps, 1, win);
  XEQ_CHECK_LAUNCH("xeq_message_wq_plan (windows)");
  const int mlong = wq_long_mult(n_edges, n_ranges);
  if (mlong > 1) {   // the long class of the l = 0 units (wq_long_mult): its window table behind the short class's
    const int n_long = wq_class_steps(n_ranges, mlong);
    hipLaunchKernelGGL(k_wq_windows, dim3((unsigned)n_long), dim3(64), 0, (hipStream_t)stream, (const int32_t*)sq,
                       (const int32_t*)pgath, n_ranges, n_long, mlong, win + 2 * n_steps);
    XEQ_CHECK_LAUNCH("xeq_message_wq_plan (windows, long class)");
  }
  return XEQ_OK;
}

int64_t xeq_message_wq_win_ints(int n_ranges) {   /* ints of the plan's window table: both stream classes (include/xeq.h) */
  return 2 * ((int64_t)wq_class_steps(n_ranges, 1) + (int64_t)wq_class_steps(n_ranges, 2) + 1);
}

static int wq_edge_basis(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                         int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1,
                         void* basis, void* dbasis, const WqTableIndex& ti, void* stream) {
  XEQ_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && num_basis >= 1 && num_basis <= 31 && cutoff > 0, "xeq_edge_basis_wq: bad sizes");
  XEQ_CHECK_ARG(rbf_kind >= XEQ_RBF_BESSEL && rbf_kind <= XEQ_RBF_EXPNORM, "xeq_edge_basis_wq: rbf kernel %d is not implemented", rbf_kind);
  XEQ_CHECK_ARG(rbf_kind == XEQ_RBF_BESSEL || p1 != nullptr, "xeq_edge_basis_wq: this radial basis needs its second parameter array (std / logc / mu)");
  XEQ_CHECK_ARG(cutoff_kind == XEQ_CUTOFF_COSINE || cutoff_kind == XEQ_CUTOFF_POLYNOMIAL, "xeq_edge_basis_wq: cutoff function %d is not implemented", cutoff_kind);
  if (n_edges == 0 && n_nodes == 0) return XEQ_OK;   // (no edge at all: the nodes' lone quads still need their zero records)
  const int64_t pcap = wq_pcap(n_nodes, n_edges), total = (pcap + WQ_REC_SLOTS - 1) / WQ_REC_SLOTS * 256;   // a workgroup per WQ_REC_SLOTS records
  const int ks = wq_ks(num_basis);
  XEQ_CHECK_ARG(pcap * wq_recf(ks) < (1ll << 31) * 2, "xeq_edge_basis_wq: too many edges for 32-bit record offsets (shard the batch)");
  RadialSpec rs{rbf_kind, cutoff_kind, num_basis, cutoff};
  hipLaunchKernelGGL(k_wq_records, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)vec,
                     peid, qptr, n_nodes, pcap, rs, (const float*)p0, (const float*)p1, (float*)basis, (float*)dbasis, wq_recf(ks), wq_tailw(ks), wq_bftail(ks) ? 1 : 0, ti);
  XEQ_CHECK_LAUNCH("xeq_edge_basis_wq");
  return XEQ_OK;
}
int xeq_edge_basis_wq(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                      int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1,
                      void* basis, void* dbasis, void* stream) {
  return wq_edge_basis(vec, n_nodes, n_edges, qptr, peid, rbf_kind, cutoff_kind, num_basis, cutoff, p0, p1, basis, dbasis, WqTableIndex{}, stream);
}
int xeq_edge_basis_wq_table(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                            int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1,
                            void* basis, void* dbasis, const int32_t* pgath, const int32_t* qinfo, const void* z, int z_is_int64,
                            int64_t table_rows, int32_t* slot_rows, int32_t* quad_rows, void* stream) {
  XEQ_CHECK_ARG(pgath && qinfo && z && slot_rows && quad_rows && table_rows >= 1, "xeq_edge_basis_wq_table: NULL argument / empty table");
  const WqTableIndex ti{z, z_is_int64, table_rows, pgath, (const uint32_t*)qinfo, slot_rows, quad_rows};
  return wq_edge_basis(vec, n_nodes, n_edges, qptr, peid, rbf_kind, cutoff_kind, num_basis, cutoff, p0, p1, basis, dbasis, ti, stream);
}

static int wq_ks_template(int num_basis) {   // the KS the dispatch macros instantiate for this basis width
  const int ks = wq_ks(num_basis);
  return ks <= 1 ? 1 : (ks <= 3 ? 3 : (ks <= 4 ? 4 : 8));
}
int64_t xeq_message_wq_packed_weight_floats(int num_basis, int node_dim, const int32_t mul[3]) {
  if (!wq_supported(num_basis, node_dim, mul)) return -1;
  const int kst = wq_ks_template(num_basis);
  const int64_t per_unit = 3 * (int64_t)(3 * 64 * 4 + (wq_bftail(kst) ? 3 * 64 * 4 : kst * 64));
  return per_unit * (mul[0] / 32 + mul[1] / 32 + mul[2] / 32);
}
int xeq_message_wq_pack_weights(const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* packed,
                                void* stream) {
  WqArgs a{};
  int rcode = wq_check("xeq_message_wq_pack_weights", 0, 0, 1, num_basis, node_dim, mul, a);
  if (rcode != XEQ_OK) return rcode;
  XEQ_CHECK_ARG(w_rbf && b_rbf && packed, "xeq_message_wq_pack_weights: NULL argument");
  const int nunits = a.nu[0] + a.nu[1] + a.nu[2];
  const dim3 grid((unsigned)nunits);
  switch (wq_ks_template(num_basis)) {
    case 1: hipLaunchKernelGGL(k_wq_pack_weights<1>, grid, dim3(256), 0, (hipStream_t)stream, a, (const float*)w_rbf, (const float*)b_rbf, (float*)packed); break;
    case 3: hipLaunchKernelGGL(k_wq_pack_weights<3>, grid, dim3(256), 0, (hipStream_t)stream, a, (const float*)w_rbf, (const float*)b_rbf, (float*)packed); break;
    case 4: hipLaunchKernelGGL(k_wq_pack_weights<4>, grid, dim3(256), 0, (hipStream_t)stream, a, (const float*)w_rbf, (const float*)b_rbf, (float*)packed); break;
    default: hipLaunchKernelGGL(k_wq_pack_weights<8>, grid, dim3(256), 0, (hipStream_t)stream, a, (const float*)w_rbf, (const float*)b_rbf, (float*)packed); break;
  }
  XEQ_CHECK_LAUNCH("xeq_message_wq_pack_weights");
  return XEQ_OK;
}

// slot_rows != NULL: the table form (h / xhat are then the element table's rows)
static int wq_message_fwd(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                          const int32_t* c_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis, const void* h,
                          const void* xhat, const void* s_in, const void* x_in, const void* w_rbf, const void* b_rbf,
                          int num_basis, int node_dim, const int32_t mul[3], void* s_out, void* x_out, int xhat_layout,
                          const int32_t* slot_rows, int64_t table_rows, void* stream) {
  WqArgs a{};
  int rcode = wq_check("xeq_message_fwd_wq", n_nodes, n_edges, n_ranges, num_basis, node_dim, mul, a);
  if (rcode != XEQ_OK) return rcode;
  if (n_nodes == 0) return XEQ_OK;
  a.sq = sq;
  a.sn = sn;
  a.rowptr = c_rowptr;
  a.pgath = slot_rows ? slot_rows : pgath;
  a.tab_rows = (int)table_rows;
  a.qinfo = (const uint32_t*)qinfo;
  a.xl = xhat_layout & 1;
  a.packed_w = (xhat_layout & XEQ_WQ_PACKED_WEIGHTS) ? 1 : 0;
  const bool x_zero = (xhat_layout & XEQ_XHAT_HIGHER_L_ZERO) != 0;
  a.win = win;
  const int nunits = a.nu[0] + a.nu[1] + a.nu[2];
  unsigned nblocks;
  wq_geometry(a, nunits, nblocks);
  dim3 grid(nblocks);
  if (slot_rows)
    XEQ_WQ_DISPATCH_TAB(k_message_fwd_wq, a, (const float*)basis, (const float*)h, (const float*)xhat, (const float*)s_in,
                        (const float*)x_in, (const float*)w_rbf, (const float*)b_rbf, (float*)s_out, (float*)x_out);
  else
    XEQ_WQ_DISPATCH(k_message_fwd_wq, x_zero, a, (const float*)basis, (const float*)h, (const float*)xhat, (const float*)s_in,
                    (const float*)x_in, (const float*)w_rbf, (const float*)b_rbf, (float*)s_out, (float*)x_out);
  XEQ_CHECK_LAUNCH(slot_rows ? "xeq_message_fwd_wq_table" : "xeq_message_fwd_wq");
  return XEQ_OK;
}
int xeq_message_fwd_wq(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                       const int32_t* c_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis, const void* h,
                       const void* xhat, const void* s_in, const void* x_in, const void* w_rbf, const void* b_rbf,
                       int num_basis, int node_dim, const int32_t mul[3], void* s_out, void* x_out, int xhat_layout,
                       void* stream) {
  return wq_message_fwd(n_nodes, n_edges, n_ranges, sq, sn, win, c_rowptr, pgath, qinfo, basis, h, xhat, s_in, x_in, w_rbf, b_rbf, num_basis,
                        node_dim, mul, s_out, x_out, xhat_layout, nullptr, 0, stream);
}
int xeq_message_fwd_wq_table(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                             const int32_t* c_rowptr, const int32_t* slot_rows, const int32_t* qinfo, const void* basis,
                             const void* h_table, const void* xhat0_table, int64_t table_rows, const void* s_in, const void* x_in,
                             const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* s_out,
                             void* x_out, int xhat_layout, void* stream) {
  XEQ_WQ_CHECK_TABLE("xeq_message_fwd_wq_table", table_rows, slot_rows, xhat_layout);
  return wq_message_fwd(n_nodes, n_edges, n_ranges, sq, sn, win, c_rowptr, nullptr, qinfo, basis, h_table, xhat0_table, s_in, x_in, w_rbf, b_rbf,
                        num_basis, node_dim, mul, s_out, x_out, xhat_layout, slot_rows, table_rows, stream);
}

/* development: read and clear the counters of a -DXEQ_WQ_ROLE_TIME_FWD / -DXEQ_WQ_STAMPS build (this object's) */
int xeq_wq_debug_wg(unsigned long long* out) { return wq_debug_wg(out); }
int xeq_wq_debug_stamps(unsigned long long out[32]) { return wq_debug_stamps(out); }

}  // extern "C"
