// Fused XPaiNN message kernels, "wave / quad" form: the reverse kernel and the edge gradients (the walk order and the arithmetic
// mapping: xeq_message_wq.hip; what both files compile: xeq_message_wq.h).  An object of its own because it is built with the default,
// register-pressure-aware machine scheduler (csrc/build.py), which orders the unfenced reverse tile better than max-ILP does.
#include "xeq_message_wq.h"

namespace xeq {

// (No scheduling fences between the quads / passes of a reverse tile since round 3: with the owner rows fetched at the tile top the
// default scheduler orders a tile's loads better than the fenced max-ILP stream did -- reverse launch 404 -> 355 us on QM9-1024.)
#ifndef XEQ_WQ_BWD_WPE
#define XEQ_WQ_BWD_WPE 2
#endif

// ------------------------------------------------------------------------------------------------ reverse
struct WqParts {
  float* pd;   // [NU][P]      per-unit partial of dL/dd, by padded slot of the reverse walk
  float* y1;   // [nu1][3][P]  per-unit partial of dL/dY_1m
  float* y2;   // [nu2][5][P]
  int64_t P;   // row length (capacity of the padded order)
};

// Sums over the 32 lanes of each half-wave for the 16 rows of a tile, as a register-halving butterfly: at every step a
// lane keeps half of its registers (chosen by one bit of its lane id) and adds the partner lane's copy of them, so
// 8 + 4 + 2 + 1 = 15 (select, select, DPP add) triples replace sixteen five-step trees.  Staged so that a quad's four
// rows collapse as soon as they exist (wq_red_ab: partners j ^ 1, j ^ 2), and the four quad results of a tile
// collapse at its end (wq_red_cd: partners j ^ 4, j ^ 8, then the other 16-lane row).  Afterwards lane j of a half
// holds the total of row  wq_red_row(j) = 4 (2 b2 + b3) + 2 b0 + b1  (b_k = bit k of j) over the half's 32 lanes.
#define XEQ_WQ_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), ctrl, 0xF, 0xF, true))
__device__ __forceinline__ float wq_red_ab(float r0, float r1, float r2, float r3, bool b0, bool b1) {
  const float a0 = (b0 ? r2 : r0) + XEQ_WQ_DPP(b0 ? r0 : r2, 0xB1);   // quad_perm [1,0,3,2]: lane j ^ 1
  const float a1 = (b0 ? r3 : r1) + XEQ_WQ_DPP(b0 ? r1 : r3, 0xB1);
  return (b1 ? a1 : a0) + XEQ_WQ_DPP(b1 ? a0 : a1, 0x4E);              // quad_perm [2,3,0,1]: lane j ^ 2
}
__device__ __forceinline__ float wq_xor4(float v) {   // lane j ^ 4: quad_perm [3,2,1,0] (j ^ 3) then row_half_mirror (j ^ 7)
  const float t = XEQ_WQ_DPP(v, 0x1B);
  return XEQ_WQ_DPP(t, 0x141);
}
__device__ __forceinline__ float wq_red_cd(float q0, float q1, float q2, float q3, bool b2, bool b3) {
  const float c0 = (b2 ? q2 : q0) + wq_xor4(b2 ? q0 : q2);
  const float c1 = (b2 ? q3 : q1) + wq_xor4(b2 ? q1 : q3);
  float r = (b3 ? c1 : c0) + XEQ_WQ_DPP(b3 ? c0 : c1, 0x128);          // row_ror:8: lane j ^ 8
  r += __shfl_xor(r, 16, 64);                                          // the half's other 16-lane row
  return r;
}
__device__ __forceinline__ int wq_red_row(int j) { return 4 * (((j >> 2) & 1) * 2 + ((j >> 3) & 1)) + 2 * (j & 1) + ((j >> 1) & 1); }

// One role of the reverse pass, in passes of two accumulators (value and d/dd filter of one kind).  Per quad the owner
// (neighbor) node's rows are constants:
//   pass S (state): u_m = sum_r phi_s[r] gx[r][m];  g_hs[n] += <xhat[n], u>;  g_xhat[n][m] += h_s[n] u_m
//                   pd[r] = h_s[n] <xhat[n], gx[r]> phi_s'[r]
//   pass E (edge):  g_he[n] += sum_r phi_e[r] <Y[r], gx[r]>;  pd[r] += h_e[n] <Y[r], gx[r]> phi_e'[r]
//                   dL/dY_m[r] = sum_ch h_e[n] phi_e[r] gx[r][m]
//   pass M (msg):   g_hm[n] += sum_r phi_m[r] gs[r];  pd[r] += h_m[n] gs[r] phi_m'[r]
// window of the reverse pass: per row (center node) the unit's run of grad_x (32 NM floats, e3nn layout) and, for l = 0,
// its 32 floats of grad_s
template <int NM>
__device__ __forceinline__ void wq_stage_bwd(const WqArgs& a, const WqUnit& un, const float* __restrict__ grad_s,
                                             const float* __restrict__ grad_x, int w0, int nrows, float* win) {
  constexpr int NSL = NM + (NM == 1 ? 1 : 0);
  const int total = nrows * NSL * 8;   // 16-byte chunks
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
      const float* src = sl < NM ? grad_x + n * a.D + un.xbase + 32 * sl : grad_s + n * a.F + 32 * un.cb;
      v[k] = *reinterpret_cast<const f32x4*>(src + 4 * chunk);
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int idx = base + k * nthr;
      if (idx < total) *reinterpret_cast<f32x4*>(win + (idx >> 3) * 32 + 4 * (idx & 7)) = v[k];
    }
  }
}

// TAB (with FIRST): the table form of the first block -- the owners' rows are rows of the element table (h, xhat_ point at h_table
// [T, H] and xhat0_table [T, F]; the quad's table row comes with its record: a.qtab, T_QTAB), read from the few cache-resident rows
// of the species present instead of from a per-node copy; the gathered gradients are per node and keep their window.
// (MEASURED AND NOT KEPT: a 24 KB window and amdgpu_waves_per_eu(3) for this form -- 165 registers, no spill, three workgroups per CU --
// ran the launch in 190 instead of 134 us on QM9-1024: the l > 0 units' steps no longer fit the window; profiles/first_block_table_timing.txt)
template <int NM, int KS, bool WIN, bool FIRST, bool TAB = false>
__device__ __forceinline__ void wq_bwd_body(const WqArgs& a, int range, int unit, const WqUnit un, const WqCols& wc,
                                            const float* __restrict__ rec, const float* __restrict__ drec,
                                            const float* __restrict__ h, const float* __restrict__ xhat_,
                                            const float* __restrict__ grad_s, const float* __restrict__ grad_x, const float* wl,
                                            float* __restrict__ grad_h, float* __restrict__ grad_xhat_, const WqParts parts,
                                            int* tbl, const float* win, int w0, unsigned long long* st_,
                                            unsigned long long& last_) {
  static_assert(!TAB || FIRST, "the table form is a first-block form");
  constexpr bool HAS_S = NM == 1;
  constexpr int YOFF = NM == 3 ? 0 : 3;
  constexpr int ROWB = (NM + (HAS_S ? 1 : 0)) * 128;
  const int lane = threadIdx.x & 63, j = lane & 31, hh = lane >> 5;
  const float* __restrict__ xhat = xhat_ + wc.x_base;
  float* __restrict__ grad_xhat = grad_xhat_ + wc.x_base;
  const uint32_t he_off = 4u * (uint32_t)a.C, row_h = 4u * (uint32_t)a.H;
  // grad_h NULL: only dL/dvec is wanted (first block of a force evaluation).  FIRST knows it at compile time (the value
  // filters, the owners' sums and their stores drop out as dead code) and knows xhat = 0 on the l > 0 columns (pass S,
  // whose every term carries a factor xhat, is not run there)
  const bool node_grads = !FIRST && grad_h != nullptr;
  wq_for_isolated(a, range, lane, [&](int m) {   // nobody's neighbor: zero gradients on the unit's columns
    if (hh == 0 && node_grads) {
      wq_st(grad_h, (uint32_t)m * row_h + wc.b_hs, 0.f);
      wq_st(grad_h, (uint32_t)m * row_h + wc.b_hs + he_off, 0.f);
      if constexpr (HAS_S) wq_st(grad_h, (uint32_t)m * row_h + wc.b_hm, 0.f);
#pragma unroll
      for (int mm = 0; mm < NM; ++mm) wq_st(grad_xhat, (uint32_t)m * wc.xnode_b + wc.b_x + mm * wc.xcomp_b, 0.f);
    }
  });
  const WqStreams st = wq_streams(a, range, un.l == 0 ? a.mlong : 1);
  if (st.ntiles == 0) return;
  // gathered rows: grad_x, grad_s of the center (window mode: one LDS row of ROWB bytes holds both)
  const uint32_t stride0 = WIN ? (uint32_t)ROWB : 4u * (uint32_t)a.D, stride1 = WIN ? (uint32_t)ROWB : 4u * (uint32_t)a.F;
  const uint32_t gbase = WIN ? (uint32_t)w0 : 0u;
  const uint32_t lgx = 4u * (uint32_t)(j * NM), lgs = (uint32_t)(NM * 128 + 4 * j);   // window mode: lane offsets in a row
  const float* Ws = wl;
  const float* We = wl + WQ_WK<KS>;
  const float* Wm = wl + 2 * WQ_WK<KS>;

  float a_hs = 0.f, a_he = 0.f, a_hm = 0.f, a_x[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) a_x[m] = 0.f;
  const int half_beg = hh ? st.q1 : st.q0, half_end = hh ? st.q2 : st.q1;
  const bool b0 = j & 1, b1 = j & 2, b2 = j & 4, b3 = j & 8;
  const int my_r = wq_red_row(j);   // the row of a tile whose channel sums this lane holds after the butterfly

  using Row = WqRow<KS, 2, (NM > 1)>;
  Row row;
  wq_row<KS, 2, (NM > 1), TAB>(a, st, lane, 0, rec, drec, row, (int)gbase);
  wq_publish<KS, 2, (NM > 1), TAB>(lane, row, stride0, stride1, tbl, gbase);
  __builtin_amdgcn_wave_barrier();

  // The owners' rows (h_state, h_edge, h_msg, xhat of the unit's columns) of a tile's four quads.  They come from GLOBAL memory (the
  // owner of a quad is the node whose gradient the wave accumulates: not a row of the window), and up to round 5 they were requested
  // inside the tile that multiplies them -- the l = 0 role in its quad loops, the l > 0 roles at the tile top: the phase stamps of
  // round 6 show the first pass of a tile (which waits for them) at 29 % of a wave's cycles against 6 % for the second.  They are now
  // requested ONE TILE AHEAD (l = 0, 1: 16 / 20 registers; the l = 2 role has no register to spare and keeps the tile-top request): as
  // soon as the next tile's table is published its owners are known, and the loads fly under the loop's back edge, the wait for the
  // next records and the first matrix chain.
  constexpr bool OWN_AHEAD = NM <= 3;
  struct Owners {
    float hs[4], he[4], hm[HAS_S ? 4 : 1], x[4][NM];
  };
  auto load_owners = [&](const int* tb_) {
    Owners o;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t own = (uint32_t)tb_[(TAB ? T_QTAB : T_QOWN) + 4 * hh + g];
      o.he[g] = wq_ld(h, own * row_h + wc.b_hs + he_off);
      if constexpr (HAS_S) o.hm[g] = wq_ld(h, own * row_h + wc.b_hm);
      if constexpr (!FIRST || HAS_S) {
        o.hs[g] = wq_ld(h, own * row_h + wc.b_hs);
        if constexpr (TAB) {   // (FIRST: l = 0 only) row `own` of xhat0_table [T, F]
          o.x[g][0] = wq_ld(xhat_, own * (4u * (uint32_t)a.F) + wc.b_hs);
        } else {
#pragma unroll
          for (int m = 0; m < NM; ++m) o.x[g][m] = wq_ld(xhat, own * wc.xnode_b + wc.b_x + m * wc.xcomp_b);
        }
      }
    }
    return o;
  };
  Owners own_next;
  if constexpr (OWN_AHEAD) own_next = load_owners(tbl);

  // The per-edge partials of a tile (dL/dd and dL/dY_lm of its sixteen rows per half) are stored at the TOP of the next tile (round 6).
  // A store inside `if (keeper)` is a memory operation that may or may not have been issued, so the compiler has to wait for the record
  // prefetch -- issued in front of it -- with s_waitcnt vmcnt(0), which waits for the store as well: at the tile's end that was the next
  // tile's first act.  Issued here they are a whole tile old when the next wait counts them.
  float pend_pd = 0.f, pend_y[NM > 1 ? NM : 1];
  int64_t pend_slot = 0;
  bool pend_keep = false;
  float pend_hm[HAS_S ? 4 : 1];          // l = 0, general form: the scalar-message gradients of the tile's finished owners (pass M)
  uint32_t pend_hm_off[HAS_S ? 4 : 1];
  bool pend_hm_last[HAS_S ? 4 : 1];
  if constexpr (HAS_S) {
#pragma unroll
    for (int g = 0; g < 4; ++g) pend_hm_last[g] = false;
  }
  // the node gradients of passes S and E are stored at the next tile's top as well (l = 0, 1; the l = 2 role has no registers for it), which
  // leaves the rows of a tile without a branch: one scheduling region with the matrix chains (OVL below)
  constexpr bool DEFER_SE = !FIRST && NM <= 3;
  float pend_hs[DEFER_SE ? 4 : 1], pend_he[DEFER_SE ? 4 : 1], pend_gx[DEFER_SE ? 4 : 1][NM];
  uint32_t pend_own[DEFER_SE ? 4 : 1];
  bool pend_se_last[DEFER_SE ? 4 : 1];
  if constexpr (DEFER_SE) {
#pragma unroll
    for (int g = 0; g < 4; ++g) pend_se_last[g] = false;
  }
  auto flush_parts = [&]() {
    if constexpr (DEFER_SE) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (pend_se_last[g]) {
          wq_st(grad_h, pend_own[g] * row_h + wc.b_hs, pend_hs[g]);
          wq_st(grad_h, pend_own[g] * row_h + wc.b_hs + he_off, pend_he[g]);
          const uint32_t ox = pend_own[g] * wc.xnode_b + wc.b_x;
#pragma unroll
          for (int m = 0; m < NM; ++m) wq_st(grad_xhat, ox + m * wc.xcomp_b, pend_gx[g][m]);
        }
    }
    if constexpr (HAS_S && !FIRST) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (pend_hm_last[g]) wq_st(grad_h, pend_hm_off[g], pend_hm[g]);
    }
    if (pend_keep) {
      parts.pd[(int64_t)unit * parts.P + pend_slot] = pend_pd;
      if constexpr (NM > 1) {
        float* dst = NM == 3 ? parts.y1 : parts.y2;
#pragma unroll
        for (int m = 0; m < NM; ++m) dst[((int64_t)un.cb * NM + m) * parts.P + pend_slot] = pend_y[m];
      }
    }
  };

  for (int t = 0; t < st.ntiles; ++t) {
    const int* tb = tbl + (t & 1) * T_SIZE;
    int* tnext = tbl + ((t + 1) & 1) * T_SIZE;
    flush_parts();   // the previous tile's partials
    const WqR<KS> R = row.R[0], Rd = row.R[1];
    WQ_STAMP(4);   // waiting for the tile's records
    // gathered gradient rows of one quad (the center's grad_x, NM components per channel)
    auto load_gx = [&](int g, float (&gxq)[4][NM]) {
      uint32_t g0[4];
      wq_tread4<uint32_t>(tb, T_G0 + 16 * hh + 4 * g, g0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < NM; ++m)
          gxq[r][m] = WIN ? wq_lds(win, g0[r] + lgx + 4u * m) : wq_ld(grad_x, g0[r] + wc.b_xe + 4u * m);
    };
    float gxs[HAS_S ? 4 : 1][4][1];   // l = 0: the tile's grad_x rows stay in registers for passes S and E
    if constexpr (HAS_S) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float tmp[4][NM];
        load_gx(g, tmp);
#pragma unroll
        for (int r = 0; r < 4; ++r) gxs[g][r][0] = tmp[r][0];
      }
    }
    float pd[16];
    // l > 0: the owners' rows (h_state, h_edge, xhat of the unit's columns) of the tile's four quads, fetched HERE, once.  Round 2
    // loaded them quad by quad inside the passes, behind scheduling fences between the quads: a load issued in a quad was waited
    // for in that quad -- twelve exposed global round trips per tile (step timeline of round 3, QM9-1024: a range of the l = 1 /
    // l = 2 units took 41 / 55 us against 28 us for l = 0, whose loads the scheduler hoists by itself; 34 / 43 us now).
    const Owners oq = OWN_AHEAD ? own_next : load_owners(tb);   // (the tile-top request where the rows are not a tile ahead)
    // (The NEXT tile's records and indices requested here, a whole tile ahead of the table that is published from them, instead of behind
    // the last matrix chain: 34 registers, no change on the whole step -- profiles/r06_small_experiments.txt item 7.)
    WQ_STAMP(5);   // tile top: gathers issued
    // l > 0: the gathered rows are read one component at a time (four rows x one m), used and dropped: out of the LDS
    // window a re-read costs 2 cycles, while holding a quad's 4 x NM values (next to the filters, pd and the per-quad
    // partial sums) spilled 114 registers in the l = 2 role
    auto gx4 = [&](const uint32_t (&g0)[4], int m, float (&gv)[4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) gv[r] = WIN ? wq_lds(win, g0[r] + lgx + 4u * m) : wq_ld(grad_x, g0[r] + wc.b_xe + 4u * m);
    };
    // The NEXT pass's matrix chains are written in front of THIS pass's rows (round 6).  With the rows free of branches (the node
    // gradients of a tile are stored at the next tile's top) a pass's rows and the next pass's chains are one scheduling region, and
    // the compiler places ~7 vector instructions between two matrix instructions instead of issuing eighteen of them back to back: a
    // wave overlaps its own matrix chains with its own row arithmetic instead of waiting for the SIMD's other wave to do so.
    // Reverse pair 432 -> 414 us (profiles/r06_small_experiments.txt item 12).  XEQ_WQ_OVERLAP_MAXNM: which roles (default l = 0, 1).
#ifndef XEQ_WQ_OVERLAP_MAXNM
#define XEQ_WQ_OVERLAP_MAXNM 3
#endif
    constexpr bool OVL = NM <= XEQ_WQ_OVERLAP_MAXNM && (DEFER_SE || (FIRST && HAS_S));
    f32x16 de_h, qe_h, dm_h, qm_h;
    if constexpr (FIRST && NM > 1) {
#pragma unroll
      for (int v = 0; v < 16; ++v) pd[v] = 0.f;
    } else {  // ---- pass S
      const f32x16 ds = wq_filter<KS>(R, Ws, lane), qs = wq_filter<KS>(Rd, Ws, lane);
      if constexpr (OVL) {   // development: the NEXT pass's chains issued in front of this pass's rows (one branch-free region: see OVL)
        de_h = wq_filter<KS>(R, We, lane);
        qe_h = wq_filter<KS>(Rd, We, lane);
      }
      WQ_STAMP(6);   // MFMA issue (all passes)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 4 * hh + g;
        const uint32_t own = (uint32_t)tb[T_QOWN + c];
        const int keep = tb[T_QKEEP + c], last = tb[T_QLAST + c];
        const float o_hs = oq.hs[g];
        float o_x[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) o_x[m] = oq.x[g][m];
        uint32_t g0[4];
        if constexpr (!HAS_S) wq_tread4<uint32_t>(tb, T_G0 + 16 * hh + 4 * g, g0);
        float u[NM], dgs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          float gv[4];
          if constexpr (HAS_S) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gv[r] = gxs[g][r][0];
          } else {
            gx4(g0, m, gv);
          }
          u[m] = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            u[m] = __builtin_fmaf(ds[4 * g + r], gv[r], u[m]);
            dgs[r] = __builtin_fmaf(o_x[m], gv[r], dgs[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pd[4 * g + r] = (o_hs * dgs[r]) * qs[4 * g + r];
        float hsq = 0.f;
#pragma unroll
        for (int m = 0; m < NM; ++m) hsq = __builtin_fmaf(o_x[m], u[m], hsq);
        a_hs = (keep ? a_hs : 0.f) + hsq;
#pragma unroll
        for (int m = 0; m < NM; ++m) a_x[m] = __builtin_fmaf(o_hs, u[m], keep ? a_x[m] : 0.f);
        if constexpr (DEFER_SE) {
          pend_hs[g] = a_hs;
#pragma unroll
          for (int m = 0; m < NM; ++m) pend_gx[g][m] = a_x[m];
          pend_own[g] = own;
          pend_se_last[g] = last && node_grads;
        } else if (last && node_grads) {
          wq_st(grad_h, own * row_h + wc.b_hs, a_hs);
          const uint32_t ox = own * wc.xnode_b + wc.b_x;
#pragma unroll
          for (int m = 0; m < NM; ++m) wq_st(grad_xhat, ox + m * wc.xcomp_b, a_x[m]);
        }
      }
    }
    WQ_STAMP(7);   // rows of pass S
    const int my_q = half_beg + 4 * t + (my_r >> 2);                   // quad of the row this lane reports
    const bool keeper = j < 16 && my_q < half_end;                     // one 16-lane row per half stores
    const int64_t my_slot = 4 * (int64_t)my_q + (my_r & 3);
    {  // ---- pass E
      const f32x16 de = OVL ? de_h : wq_filter<KS>(R, We, lane), qe = OVL ? qe_h : wq_filter<KS>(Rd, We, lane);
      if constexpr (OVL && HAS_S) {
        dm_h = wq_filter<KS>(R, Wm, lane);
        qm_h = wq_filter<KS>(Rd, Wm, lane);
      }
      WQ_STAMP(6);
      float pq[NM > 1 ? NM : 1][4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int p0 = 16 * hh + 4 * g, c = 4 * hh + g;
        const uint32_t own = (uint32_t)tb[T_QOWN + c];
        const int keep = tb[T_QKEEP + c], last = tb[T_QLAST + c];
        const float o_he = oq.he[g];
        uint32_t g0[4];
        if constexpr (!HAS_S) wq_tread4<uint32_t>(tb, T_G0 + p0, g0);
        float dge[4], heq = 0.f;   // dge[r] = <Y[r], gx[r]>, one component at a time
#pragma unroll
        for (int r = 0; r < 4; ++r) dge[r] = NM > 1 ? 0.f : gxs[HAS_S ? g : 0][r][0];
        if constexpr (NM > 1) {
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            float Ym[4], gv[4];
            wq_tread4<float>(tb, T_Y + 32 * (YOFF + m) + p0, Ym);
            gx4(g0, m, gv);
#pragma unroll
            for (int r = 0; r < 4; ++r) dge[r] = __builtin_fmaf(Ym[r], gv[r], dge[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = 4 * g + r;
          heq = __builtin_fmaf(de[v], dge[r], heq);
          pd[v] = __builtin_fmaf(o_he * dge[r], qe[v], pd[v]);
        }
        a_he = (keep ? a_he : 0.f) + heq;
        if constexpr (DEFER_SE) pend_he[g] = a_he;
        else if (last && node_grads) wq_st(grad_h, own * row_h + wc.b_hs + he_off, a_he);
      }
      if constexpr (NM > 1) {
        // dL/dY_lm of every row's edge, in a second walk over the quads: the d/dd filter is dead by now, which is the
        // room the per-quad partial sums need (one walk spilled 48 registers in the l = 2 role)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int p0 = 16 * hh + 4 * g;
          const float o_he = oq.he[g];
          uint32_t g0[4];
          wq_tread4<uint32_t>(tb, T_G0 + p0, g0);
          float wy[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) wy[r] = o_he * de[4 * g + r];
#pragma unroll
          for (int m = 0; m < NM; ++m) {   // first half of the sum over the unit's 32 channels
            float gv[4];
            gx4(g0, m, gv);
            pq[m][g] = wq_red_ab(wy[0] * gv[0], wy[1] * gv[1], wy[2] * gv[2], wy[3] * gv[3], b0, b1);
          }
        }
      }
      if constexpr (NM > 1) {
#pragma unroll
        for (int m = 0; m < NM; ++m) pend_y[m] = wq_red_cd(pq[m][0], pq[m][1], pq[m][2], pq[m][3], b2, b3);
      }
    }
    if constexpr (!HAS_S) wq_row<KS, 2, (NM > 1), TAB>(a, st, lane, t + 1, rec, drec, row, (int)gbase);   // next tile's records
    WQ_STAMP(8);   // rows of pass E (+ dL/dY sums)
    if constexpr (HAS_S) {  // ---- pass M
      float gsv[16];          // the centers' grad_s rows: only this pass reads them; they land under its MFMAs
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t g1[4];
        wq_tread4<uint32_t>(tb, T_G1 + 16 * hh + 4 * g, g1);
#pragma unroll
        for (int r = 0; r < 4; ++r) gsv[4 * g + r] = WIN ? wq_lds(win, g1[r] + lgs) : wq_ld(grad_s, g1[r] + wc.b_s);
      }
      const f32x16 dm = (OVL && HAS_S) ? dm_h : wq_filter<KS>(R, Wm, lane), qm = (OVL && HAS_S) ? qm_h : wq_filter<KS>(Rd, Wm, lane);
      wq_row<KS, 2, (NM > 1), TAB>(a, st, lane, t + 1, rec, drec, row, (int)gbase);   // last MFMAs issued: next tile's records
      WQ_STAMP(6);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 4 * hh + g;
        const uint32_t own = (uint32_t)tb[T_QOWN + c];
        const int keep = tb[T_QKEEP + c], last = tb[T_QLAST + c];
        const float o_hm = oq.hm[HAS_S ? g : 0];
        float hmq = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = 4 * g + r;
          hmq = __builtin_fmaf(dm[v], gsv[v], hmq);
          pd[v] = __builtin_fmaf(o_hm * gsv[v], qm[v], pd[v]);
        }
        a_hm = (keep ? a_hm : 0.f) + hmq;
        if constexpr (!FIRST) {   // (this pass's stores come BEHIND the next tile's record request: to the next tile's top with the partials)
          pend_hm[g] = a_hm;
          pend_hm_off[g] = own * row_h + wc.b_hm;
          pend_hm_last[g] = last && node_grads;
        } else if (last && node_grads) wq_st(grad_h, own * row_h + wc.b_hm, a_hm);
      }
    }
    WQ_STAMP(9);   // rows of pass M
    {  // ---- dL/dd of every row's edge: sum over the unit's 32 channels
      float pq[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) pq[g] = wq_red_ab(pd[4 * g], pd[4 * g + 1], pd[4 * g + 2], pd[4 * g + 3], b0, b1);
      const float tot = wq_red_cd(pq[0], pq[1], pq[2], pq[3], b2, b3);
      pend_pd = tot;
      pend_slot = my_slot;
      pend_keep = keeper;
    }
    WQ_STAMP(11);  // dL/dd channel sums
    wq_publish<KS, 2, (NM > 1), TAB>(lane, row, stride0, stride1, tnext, gbase);
    __builtin_amdgcn_wave_barrier();
    if constexpr (OWN_AHEAD) own_next = load_owners(tnext);   // the next tile's owners are known: their rows fly under the back edge
    WQ_STAMP(12);  // next table published
  }
  flush_parts();   // the last tile's
}

template <int NM, int KS, bool FIRST, bool TAB = false>
__device__ __forceinline__ void wq_bwd_role(const WqArgs& a, int s_beg, int s_end, int unit, const WqUnit un, const float* __restrict__ rec,
                                            const float* __restrict__ drec, const float* __restrict__ h,
                                            const float* __restrict__ xhat, const float* __restrict__ grad_s,
                                            const float* __restrict__ grad_x, const float* wl, float* __restrict__ grad_h,
                                            float* __restrict__ grad_xhat, const WqParts parts, int* tbl, float* win) {
  constexpr int ROWB = (NM + (NM == 1 ? 1 : 0)) * 128;
  const WqCols wc = wq_cols<NM>(a, un, threadIdx.x & 31);
  unsigned long long st_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = 0;
#ifdef XEQ_WQ_STAMPS
  last_ = __builtin_amdgcn_s_memtime();
#endif
  const WqClass cl = wq_class(a, un.l);   // (as in the forward role: the chunk counts units, the loop the steps of this unit's class)
  const int c_beg = cl.m == a.mlong ? s_beg : s_beg * a.mlong, c_end = min(cl.m == a.mlong ? s_end : s_end * a.mlong, cl.n_steps);
  for (int step = c_beg; step < c_end; ++step) {
    const int w0 = cl.win[2 * step], nrows = cl.win[2 * step + 1];
    const bool use_win = nrows > 0 && nrows * ROWB <= WQ_WIN_FLOATS * 4;   // workgroup-uniform
    WQ_STAMP(0);
    if (use_win) wq_stage_bwd<NM>(a, un, grad_s, grad_x, w0, nrows, win);
    WQ_STAMP(1);
    __syncthreads();
    WQ_STAMP(2);
    const int range = step * WQ_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: the stream bounds become scalar loads)
    if (range < cl.n_ranges) {
      if (use_win) wq_bwd_body<NM, KS, true, FIRST, TAB>(a, range, unit, un, wc, rec, drec, h, xhat, grad_s, grad_x, wl, grad_h, grad_xhat, parts, tbl, win, w0, st_, last_);
      else wq_bwd_body<NM, KS, false, FIRST, TAB>(a, range, unit, un, wc, rec, drec, h, xhat, grad_s, grad_x, wl, grad_h, grad_xhat, parts, tbl, win, 0, st_, last_);
    }
    WQ_STAMP(3);
    __syncthreads();
    WQ_STAMP(10);
  }
#ifdef XEQ_WQ_STAMPS
#ifndef XEQ_WQ_STAMP_L
#define XEQ_WQ_STAMP_L 0
#endif
  if (NM == 2 * XEQ_WQ_STAMP_L + 1 && (threadIdx.x & 63) == 0) {   // reverse-kernel stamps go to slots 16..31 of the counter array
    for (int i = 0; i < 13; ++i) atomicAdd(&g_wq_stamps[16 + i], st_[i]);
    atomicAdd(&g_wq_stamps[31], 1ull);
  }
#endif
}

// FIRST: the model's first message block in a force evaluation -- no node gradients are wanted (grad_h, grad_xhat NULL)
// and xhat is zero on every l > 0 column
template <int KS, bool FIRST, bool TAB = false>
__global__ void __launch_bounds__(64 * WQ_WAVES) __attribute__((amdgpu_waves_per_eu(XEQ_WQ_BWD_WPE)))
k_message_bwd_wq(WqArgs a, const float* __restrict__ rec, const float* __restrict__ drec, const float* __restrict__ h,
                 const float* __restrict__ xhat, const float* __restrict__ grad_s, const float* __restrict__ grad_x,
                 const float* __restrict__ w_rbf, const float* __restrict__ b_rbf, float* __restrict__ grad_h,
                 float* __restrict__ grad_xhat, WqParts parts) {
  __shared__ __attribute__((aligned(16))) float win[WQ_WIN_FLOATS];
  __shared__ __attribute__((aligned(16))) int tbl_all[WQ_WAVES][2 * T_SIZE];
  __shared__ __attribute__((aligned(16))) float wl[3 * WQ_WK<KS>];
  int s_beg, s_end, unit;
  wq_decode(a, a.nu[0] + a.nu[1] + a.nu[2], s_beg, s_end, unit);
  if (s_beg >= s_end) return;   // padding block of the grid / empty chunk of a short region (workgroup-uniform)
  const WqUnit un = wq_unit(a, unit);
  wq_stage_weights<KS>(a, un, w_rbf, b_rbf, wl);
  __syncthreads();
  int* tbl = tbl_all[threadIdx.x >> 6];
#ifdef XEQ_WQ_ROLE_TIME   // development: where and when every workgroup of the production body ran
  unsigned long long rr0_;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rr0_)::"memory");
#endif
  if (un.l == 0) wq_bwd_role<1, KS, FIRST, TAB>(a, s_beg, s_end, unit, un, rec, drec, h, xhat, grad_s, grad_x, wl, grad_h, grad_xhat, parts, tbl, win);
  else if (un.l == 1) wq_bwd_role<3, KS, FIRST, TAB>(a, s_beg, s_end, unit, un, rec, drec, h, xhat, grad_s, grad_x, wl, grad_h, grad_xhat, parts, tbl, win);
  else wq_bwd_role<5, KS, FIRST, TAB>(a, s_beg, s_end, unit, un, rec, drec, h, xhat, grad_s, grad_x, wl, grad_h, grad_xhat, parts, tbl, win);
#ifdef XEQ_WQ_ROLE_TIME
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

// dL/dvec from the per-unit partials (by padded slot of the reverse walk), summed in unit order (deterministic),
// chain rule of A1-A3; one thread per padded slot, pads skipped
__global__ void k_wq_edge_grad(const float* __restrict__ vec, const int32_t* __restrict__ peid, const int32_t* __restrict__ mirror,
                               const int32_t* __restrict__ qptr, int64_t N, int64_t P, int nu, int nu1, int nu2,
                               const float* __restrict__ pd, const float* __restrict__ y1, const float* __restrict__ y2,
                               float* __restrict__ grad_vec) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P || p >= 4 * (int64_t)qptr[N]) return;
  int32_t e = peid[p];
  if (e < 0) return;
  if (mirror) {                // mirror walk: the slot's partials belong to the reverse edge
    const int32_t m = mirror[e];
    if (m < 0) {               // no reverse edge in the list (a periodic list one rounding off symmetric): nobody stands for edge e either
      grad_vec[3 * (int64_t)e] = grad_vec[3 * (int64_t)e + 1] = grad_vec[3 * (int64_t)e + 2] = 0.f;
      return;
    }
    e = m;
  }
  float gd = 0.f, q1[3] = {0.f, 0.f, 0.f}, q2[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int u = 0; u < nu; ++u) gd += pd[(int64_t)u * P + p];
  for (int u = 0; u < nu1; ++u)
#pragma unroll
    for (int m = 0; m < 3; ++m) q1[m] += y1[((int64_t)u * 3 + m) * P + p];
  for (int u = 0; u < nu2; ++u)
#pragma unroll
    for (int m = 0; m < 5; ++m) q2[m] += y2[((int64_t)u * 5 + m) * P + p];
  const EdgeGeom<float> g = edge_geom<float>(vec[3 * (int64_t)e], vec[3 * (int64_t)e + 1], vec[3 * (int64_t)e + 2]);
  float out[3];
  edge_grad<float>(g, gd, q1, q2, out);
  grad_vec[3 * (int64_t)e] = out[0];
  grad_vec[3 * (int64_t)e + 1] = out[1];
  grad_vec[3 * (int64_t)e + 2] = out[2];
}

// The same for ALL message blocks of an evaluation at once (round 5): the chain rule A1-A3 is linear in (dL/dd, dL/dY_1, dL/dY_2), so
// the blocks' partials are added first -- per quantity in the order the parts are listed, then over the units -- and the chain rule
// runs once: one launch per evaluation instead of one per block plus the sums of their [E, 3] results (three k_wq_edge_grad and two
// elementwise adds per force evaluation before).
struct WqPartList {
  const float* p[XEQ_WQ_MAX_PART_SETS];
  int n;
};
__global__ void k_wq_edge_grad_sum(const float* __restrict__ vec, const int32_t* __restrict__ peid, const int32_t* __restrict__ mirror,
                                   const int32_t* __restrict__ qptr, int64_t N, int64_t P, int nu, int nu1, int nu2, const WqPartList pl,
                                   float* __restrict__ grad_vec) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P || p >= 4 * (int64_t)qptr[N]) return;
  int32_t e = peid[p];
  if (e < 0) return;
  if (mirror) {
    const int32_t m = mirror[e];
    if (m < 0) {   // no mirror edge in the list (a periodic list one rounding off symmetric): then nobody stands for edge e either
      grad_vec[3 * (int64_t)e] = grad_vec[3 * (int64_t)e + 1] = grad_vec[3 * (int64_t)e + 2] = 0.f;
      return;
    }
    e = m;
  }
  float gd = 0.f, q1[3] = {0.f, 0.f, 0.f}, q2[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < pl.n; ++s) {
    const float* pd = pl.p[s];
    const float* y1 = pd + (int64_t)nu * P;
    const float* y2 = y1 + (int64_t)nu1 * 3 * P;
    for (int u = 0; u < nu; ++u) gd += pd[(int64_t)u * P + p];
    for (int u = 0; u < nu1; ++u)
#pragma unroll
      for (int m = 0; m < 3; ++m) q1[m] += y1[((int64_t)u * 3 + m) * P + p];
    for (int u = 0; u < nu2; ++u)
#pragma unroll
      for (int m = 0; m < 5; ++m) q2[m] += y2[((int64_t)u * 5 + m) * P + p];
  }
  const EdgeGeom<float> g = edge_geom<float>(vec[3 * (int64_t)e], vec[3 * (int64_t)e + 1], vec[3 * (int64_t)e + 2]);
  float out[3];
  edge_grad<float>(g, gd, q1, q2, out);
  grad_vec[3 * (int64_t)e] = out[0];
  grad_vec[3 * (int64_t)e + 1] = out[1];
  grad_vec[3 * (int64_t)e + 2] = out[2];
}


}  // namespace xeq

using namespace xeq;

extern "C" {

int64_t xeq_message_wq_parts_floats(int64_t n_nodes, int64_t n_edges, const int32_t mul[3]) {
  return wq_pcap(n_nodes, n_edges) * (int64_t)(mul[0] / 32 + mul[1] / 32 + mul[2] / 32 + 3 * (mul[1] / 32) + 5 * (mul[2] / 32));
}

// quad_rows != NULL: the table form (h / xhat are then the element table's rows; no node gradients)
static int wq_message_bwd(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                          const int32_t* n_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis,
                          const void* dbasis, const void* h, const void* xhat, const void* grad_s, const void* grad_x,
                          const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* grad_h,
                          void* grad_xhat, void* parts, int xhat_layout, const int32_t* quad_rows, int64_t table_rows, void* stream) {
  WqArgs a{};
  int rcode = wq_check("xeq_message_bwd_wq", n_nodes, n_edges, n_ranges, num_basis, node_dim, mul, a);
  if (rcode != XEQ_OK) return rcode;
  if (n_nodes == 0) return XEQ_OK;
  a.sq = sq;
  a.sn = sn;
  a.rowptr = n_rowptr;
  a.pgath = pgath;
  a.qinfo = (const uint32_t*)qinfo;
  a.qtab = quad_rows;
  a.tab_rows = (int)table_rows;
  a.xl = xhat_layout & 1;
  a.mirror = (xhat_layout & XEQ_WQ_MIRROR_WALK) ? 1 : 0;
  a.packed_w = (xhat_layout & XEQ_WQ_PACKED_WEIGHTS) ? 1 : 0;
  const bool first = (xhat_layout & XEQ_XHAT_HIGHER_L_ZERO) != 0 && grad_h == nullptr;
  const int nunits = a.nu[0] + a.nu[1] + a.nu[2];
  WqParts pr;
  pr.P = a.pcap;
  pr.pd = (float*)parts;
  pr.y1 = pr.pd + (int64_t)nunits * pr.P;
  pr.y2 = pr.y1 + (int64_t)a.nu[1] * 3 * pr.P;
  a.win = win;
  unsigned nblocks;
  wq_geometry(a, nunits, nblocks);
  dim3 grid(nblocks);
  if (quad_rows)
    XEQ_WQ_DISPATCH_TAB(k_message_bwd_wq, a, (const float*)basis, (const float*)dbasis, (const float*)h, (const float*)xhat,
                        (const float*)grad_s, (const float*)grad_x, (const float*)w_rbf, (const float*)b_rbf, (float*)nullptr,
                        (float*)nullptr, pr);
  else
    XEQ_WQ_DISPATCH(k_message_bwd_wq, first, a, (const float*)basis, (const float*)dbasis, (const float*)h, (const float*)xhat,
                    (const float*)grad_s, (const float*)grad_x, (const float*)w_rbf, (const float*)b_rbf, (float*)grad_h,
                    (float*)grad_xhat, pr);
  XEQ_CHECK_LAUNCH(quad_rows ? "xeq_message_bwd_wq_table" : "xeq_message_bwd_wq");
  return XEQ_OK;
}
int xeq_message_bwd_wq(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                       const int32_t* n_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis,
                       const void* dbasis, const void* h, const void* xhat, const void* grad_s, const void* grad_x,
                       const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* grad_h,
                       void* grad_xhat, void* parts, int xhat_layout, void* stream) {
  return wq_message_bwd(n_nodes, n_edges, n_ranges, sq, sn, win, n_rowptr, pgath, qinfo, basis, dbasis, h, xhat, grad_s, grad_x, w_rbf, b_rbf,
                        num_basis, node_dim, mul, grad_h, grad_xhat, parts, xhat_layout, nullptr, 0, stream);
}
int xeq_message_bwd_wq_table(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                             const int32_t* n_rowptr, const int32_t* pgath, const int32_t* qinfo, const int32_t* quad_rows,
                             const void* basis, const void* dbasis, const void* h_table, const void* xhat0_table, int64_t table_rows,
                             const void* grad_s, const void* grad_x, const void* w_rbf, const void* b_rbf, int num_basis, int node_dim,
                             const int32_t mul[3], void* parts, int xhat_layout, void* stream) {
  XEQ_WQ_CHECK_TABLE("xeq_message_bwd_wq_table", table_rows, quad_rows, xhat_layout);
  return wq_message_bwd(n_nodes, n_edges, n_ranges, sq, sn, win, n_rowptr, pgath, qinfo, basis, dbasis, h_table, xhat0_table, grad_s, grad_x, w_rbf,
                        b_rbf, num_basis, node_dim, mul, nullptr, nullptr, parts, xhat_layout, quad_rows, table_rows, stream);
}

/* development: read and clear the counters of a -DXEQ_WQ_ROLE_TIME / -DXEQ_WQ_STAMPS build (this object's) */
int xeq_wq_debug_wg_bwd(unsigned long long* out) { return wq_debug_wg(out); }
int xeq_wq_debug_stamps_bwd(unsigned long long out[32]) { return wq_debug_stamps(out); }

int xeq_message_wq_edge_grad(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                             const int32_t* mirror, const int32_t mul[3], const void* parts, void* grad_vec, void* stream) {
  XEQ_CHECK_ARG(n_edges >= 0 && mul[0] % 32 == 0 && mul[1] % 32 == 0 && mul[2] % 32 == 0, "xeq_message_wq_edge_grad: bad sizes");
  if (n_edges == 0) return XEQ_OK;
  const int64_t P = wq_pcap(n_nodes, n_edges);
  const int nu1 = mul[1] / 32, nu2 = mul[2] / 32, nunits = mul[0] / 32 + nu1 + nu2;
  const float* pd = (const float*)parts;
  const float* y1 = pd + (int64_t)nunits * P;
  const float* y2 = y1 + (int64_t)nu1 * 3 * P;
  hipLaunchKernelGGL(k_wq_edge_grad, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)vec,
                     peid, mirror, qptr, n_nodes, P, nunits, nu1, nu2, pd, y1, y2, (float*)grad_vec);
  XEQ_CHECK_LAUNCH("xeq_message_wq_edge_grad");
  return XEQ_OK;
}

int xeq_message_wq_edge_grad_sum(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                                 const int32_t* mirror, const int32_t mul[3], int n_sets, const void* const* parts, void* grad_vec,
                                 void* stream) {
  XEQ_CHECK_ARG(n_edges >= 0 && mul[0] % 32 == 0 && mul[1] % 32 == 0 && mul[2] % 32 == 0, "xeq_message_wq_edge_grad_sum: bad sizes");
  XEQ_CHECK_ARG(n_sets >= 1 && n_sets <= XEQ_WQ_MAX_PART_SETS && parts, "xeq_message_wq_edge_grad_sum: 1 .. %d sets of partials", XEQ_WQ_MAX_PART_SETS);
  if (n_edges == 0) return XEQ_OK;
  const int64_t P = wq_pcap(n_nodes, n_edges);
  const int nu1 = mul[1] / 32, nu2 = mul[2] / 32, nunits = mul[0] / 32 + nu1 + nu2;
  WqPartList pl;
  pl.n = n_sets;
  for (int s = 0; s < XEQ_WQ_MAX_PART_SETS; ++s) pl.p[s] = s < n_sets ? (const float*)parts[s] : nullptr;
  for (int s = 0; s < n_sets; ++s) XEQ_CHECK_ARG(pl.p[s], "xeq_message_wq_edge_grad_sum: parts[%d] is NULL", s);
  hipLaunchKernelGGL(k_wq_edge_grad_sum, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)vec,
                     peid, mirror, qptr, n_nodes, P, nunits, nu1, nu2, pl, (float*)grad_vec);
  XEQ_CHECK_LAUNCH("xeq_message_wq_edge_grad_sum");
  return XEQ_OK;
}

}  // extern "C"
