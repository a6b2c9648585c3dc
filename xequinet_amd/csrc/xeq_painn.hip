// PaiNN message and update blocks (gfx950, f32) -- the reference's nn/painn.py:
//   message  nn/painn.py:99-117   filter = (rbf W^T + b) fcut, m_s / m_v, index_add over centers, residual
//   update   nn/painn.py:146-164  U, V, |V|, <U, V>, the a_ss / a_vv / a_sv products, residual
// The scalar MLPs of both blocks (painn.py:99, :154) are the library's xeq_mlp2_fwd / _bwd launches.
//
// Layout: node scalars s [N, F], node vectors x [N, 3, F] Cartesian in x, y, z order (what the reference's modules exchange).
// Every matrix product is the exact-f32 matrix instruction v_mfma_f32_16x16x4_f32 (A[l & 15][k = l >> 4], B[k = l >> 4][l & 15],
// C: column l & 15, rows 4 (l >> 4) + r): one fused-multiply-add chain in k order per output element, so a row gets the same bits
// in any batch and in the few-row launch shapes.
//
// Message kernels: one wave per destination node walks its CSR segment in chunks of 16 edges.  Lanes 0..15 form the chunk's radial
// basis times envelope (plus one constant column that carries the bias) in LDS; the filter [16, 3F] = basis [16, B + 1] x packed
// weights [B + 1, 3F] comes out of the matrix cores 16 channels at a time and is consumed in registers.  Per-channel sums live in
// the wave's LDS slice (one slot per lane and channel block), are reduced over the four edge groups of the C layout at the end and
// stored once per node with the residual added: no atomics, a fixed summation order.  rbf[E, B], fcut[E] and the unit vectors
// never exist in memory.
#include "xeq_packed_w.h"

namespace xeq {
namespace painn {

constexpr int CHUNK = 16;        // edges per staged chunk (rows of one matrix-core tile)
constexpr int KPAD = 32;         // padded basis width: num_basis + 1 (bias column) <= 32
constexpr int BROW = KPAD + 4;   // LDS row stride of the staged basis (floats)
constexpr int TILE = 16;         // nodes per tile of the update kernels
constexpr int64_t FEW_ROWS = 2048;   // node count up to which the update products launch one wave per (tile, 16 columns)

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct MsgArgs {
  int64_t n_nodes, n_edges;
  const int32_t* rowptr;     // [N + 1] CSR over the walked row (centers forward, neighbours reverse)
  const int32_t* perm;       // slot -> edge id, or null (identity)
  const int64_t* edge_index; // [2, E]
  const float* vec;          // [E, 3]
  const float* h;            // [N, 3F] scalar_mlp output
  const float* s;            // [N, F]      (forward)
  const float* x;            // [N, 3, F]
  const float* wp;           // [KPAD, 3F] packed filter weights, row num_basis = bias, rows behind it zero
  const float* p0;
  const float* p1;
  int rbf_kind, cutoff_kind, num_basis;
  float cutoff;
  int F;
  float* s_out;              // forward outputs
  float* x_out;
  const float* g_s;          // reverse inputs (g_x may be null: zero)
  const float* g_x;
  float* g_h;                // reverse outputs (g_x_in may be null: not wanted)
  float* g_x_in;
  float* g_vec;
  int accumulate_vec;
};

// basis row of one edge: rho_k(d) f(d) for k < B, f(d) in column B (bias), zero behind; optionally the d-derivative of the same row
template <bool DERIV>
__device__ __forceinline__ void stage_edge(const MsgArgs& a, float rx, float ry, float rz, float* brow, float* drow, float* urow) {
  const EdgeGeom<float> g = edge_geom<float>(rx, ry, rz);
  float f, df;
  envelope<float>(a.cutoff_kind, g.d, a.cutoff, f, df);
  for (int k = 0; k < a.num_basis; ++k) {
    float rho, drho;
    radial<float>(a.rbf_kind, g.d, a.cutoff, a.p0[k], a.p1 ? a.p1[k] : 0.f, rho, drho, k, a.num_basis);
    brow[k] = rho * f;
    if (DERIV) drow[k] = drho * f + rho * df;
  }
  brow[a.num_basis] = f;
  if (DERIV) drow[a.num_basis] = df;
  for (int k = a.num_basis + 1; k < KPAD; ++k) {
    brow[k] = 0.f;
    if (DERIV) drow[k] = 0.f;
  }
  urow[0] = g.x;
  urow[1] = g.y;
  urow[2] = g.z;
  if (DERIV) urow[3] = g.d > 1e-12f ? g.inv_d : 0.f;
}

// ---- message forward (painn.py:99-117) --------------------------------------------------------------------------------------------
// LDS per wave: basis [CHUNK][BROW] | u [CHUNK][4] | nbr [CHUNK] | acc [4][F / 16][64]
__global__ void __launch_bounds__(256) k_message_fwd(MsgArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int F = a.F, ncb = F >> 4, ks_n = (a.num_basis + 1 + 3) >> 2;
  const int per_wave = CHUNK * BROW + CHUNK * 4 + CHUNK + 4 * ncb * 64;
  float* basis = lds + (size_t)wave * per_wave;
  float* uvec = basis + CHUNK * BROW;
  int* nbr = reinterpret_cast<int*>(uvec + CHUNK * 4);
  float* acc = reinterpret_cast<float*>(nbr + CHUNK);
  const int64_t i = (int64_t)blockIdx.x * nw + wave;
  if (i >= a.n_nodes) return;   // (whole wave; no workgroup barrier below)
  const int col = lane & 15, grp = lane >> 4;
  for (int q = lane; q < 4 * ncb * 64; q += 64) acc[q] = 0.f;
  const int k0 = a.rowptr[i], k1 = a.rowptr[i + 1];
  for (int kc = k0; kc < k1; kc += CHUNK) {
    __builtin_amdgcn_wave_barrier();
    if (lane < CHUNK) {
      const int k = kc + lane;
      if (k < k1) {
        const int64_t e = a.perm ? a.perm[k] : k;
        nbr[lane] = (int)a.edge_index[a.n_edges + e];
        stage_edge<false>(a, a.vec[3 * e], a.vec[3 * e + 1], a.vec[3 * e + 2], basis + lane * BROW, nullptr, uvec + lane * 4);
      } else {   // padding row: zero filter, a readable neighbour
        nbr[lane] = (int)i;
        for (int k = 0; k < KPAD; ++k) basis[lane * BROW + k] = 0.f;
        uvec[lane * 4] = uvec[lane * 4 + 1] = uvec[lane * 4 + 2] = 0.f;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float av[KPAD / 4];
#pragma unroll
    for (int ks = 0; ks < KPAD / 4; ++ks) av[ks] = basis[col * BROW + ks * 4 + grp];
    for (int cb = 0; cb < ncb; ++cb) {
      const int f = cb * 16 + col;
      f32x4 fs = {0.f, 0.f, 0.f, 0.f}, fe = fs, ft = fs;
#pragma unroll
      for (int ks = 0; ks < KPAD / 4; ++ks) {
        if (ks < ks_n) {
          const float* w = a.wp + (size_t)(ks * 4 + grp) * 3 * F + f;
          fs = mfma(av[ks], w[0], fs);
          fe = mfma(av[ks], w[F], fe);
          ft = mfma(av[ks], w[2 * F], ft);
        }
      }
      float as = acc[(0 * ncb + cb) * 64 + lane], a0 = acc[(1 * ncb + cb) * 64 + lane], a1 = acc[(2 * ncb + cb) * 64 + lane],
            a2 = acc[(3 * ncb + cb) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = grp * 4 + r;
        const int64_t j = nbr[row];
        const float* hj = a.h + j * 3 * F + f;
        const float* xj = a.x + j * 3 * F + f;
        const float ge = hj[F] * fe[r], gt = hj[2 * F] * ft[r];
        as += hj[0] * fs[r];
        a0 += xj[0] * gt + uvec[row * 4] * ge;
        a1 += xj[F] * gt + uvec[row * 4 + 1] * ge;
        a2 += xj[2 * F] * gt + uvec[row * 4 + 2] * ge;
      }
      acc[(0 * ncb + cb) * 64 + lane] = as;
      acc[(1 * ncb + cb) * 64 + lane] = a0;
      acc[(2 * ncb + cb) * 64 + lane] = a1;
      acc[(3 * ncb + cb) * 64 + lane] = a2;
    }
  }
  // the four edge groups of every channel, then one store per node with the residual
  for (int cb = 0; cb < ncb; ++cb) {
    const int f = cb * 16 + col;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = acc[(q * ncb + cb) * 64 + lane];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (grp == 0) {
        if (q == 0) a.s_out[i * F + f] = a.s[i * F + f] + v;
        else a.x_out[i * 3 * F + (q - 1) * F + f] = a.x[i * 3 * F + (q - 1) * F + f] + v;
      }
    }
  }
}

// ---- message reverse ---------------------------------------------------------------------------------------------------------------
// One wave per SOURCE node j walks the edges it is the neighbour of (the reverse-edge map of a symmetric list, else the
// neighbour-sorted view): dL/dh[j], dL/dx[j] summed in the wave and stored once; dL/dvec of every walked edge has this one writer.
// LDS per wave: basis [CHUNK][BROW] | dbasis [CHUNK][BROW] | u, 1/d [CHUNK][4] | ctr [CHUNK] | eid [CHUNK] | acc [6][F / 16][64]
__global__ void __launch_bounds__(128) k_message_bwd(MsgArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int F = a.F, ncb = F >> 4, ks_n = (a.num_basis + 1 + 3) >> 2;
  const int per_wave = 2 * CHUNK * BROW + CHUNK * 4 + 2 * CHUNK + 6 * ncb * 64;
  float* basis = lds + (size_t)wave * per_wave;
  float* dbasis = basis + CHUNK * BROW;
  float* uvec = dbasis + CHUNK * BROW;
  int* ctr = reinterpret_cast<int*>(uvec + CHUNK * 4);
  int* eid = ctr + CHUNK;
  float* acc = reinterpret_cast<float*>(eid + CHUNK);
  const int64_t j = (int64_t)blockIdx.x * nw + wave;
  if (j >= a.n_nodes) return;
  const int col = lane & 15, grp = lane >> 4;
  for (int q = lane; q < 6 * ncb * 64; q += 64) acc[q] = 0.f;
  const int k0 = a.rowptr[j], k1 = a.rowptr[j + 1];
  for (int kc = k0; kc < k1; kc += CHUNK) {
    __builtin_amdgcn_wave_barrier();
    if (lane < CHUNK) {
      const int k = kc + lane;
      if (k < k1) {
        const int64_t e = a.perm ? a.perm[k] : k;
        eid[lane] = (int)e;
        ctr[lane] = (int)a.edge_index[e];
        stage_edge<true>(a, a.vec[3 * e], a.vec[3 * e + 1], a.vec[3 * e + 2], basis + lane * BROW, dbasis + lane * BROW, uvec + lane * 4);
      } else {
        eid[lane] = -1;
        ctr[lane] = (int)j;
        for (int k = 0; k < KPAD; ++k) basis[lane * BROW + k] = dbasis[lane * BROW + k] = 0.f;
        uvec[lane * 4] = uvec[lane * 4 + 1] = uvec[lane * 4 + 2] = uvec[lane * 4 + 3] = 0.f;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float av[KPAD / 4], dv[KPAD / 4];
#pragma unroll
    for (int ks = 0; ks < KPAD / 4; ++ks) {
      av[ks] = basis[col * BROW + ks * 4 + grp];
      dv[ks] = dbasis[col * BROW + ks * 4 + grp];
    }
    float gd[4] = {0.f, 0.f, 0.f, 0.f}, gu0[4] = {0.f, 0.f, 0.f, 0.f}, gu1[4] = {0.f, 0.f, 0.f, 0.f}, gu2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int cb = 0; cb < ncb; ++cb) {
      const int f = cb * 16 + col;
      f32x4 fs = {0.f, 0.f, 0.f, 0.f}, fe = fs, ft = fs, ds = fs, de = fs, dt = fs;
#pragma unroll
      for (int ks = 0; ks < KPAD / 4; ++ks) {
        if (ks < ks_n) {
          const float* w = a.wp + (size_t)(ks * 4 + grp) * 3 * F + f;
          const float w0 = w[0], w1 = w[F], w2 = w[2 * F];
          fs = mfma(av[ks], w0, fs);
          fe = mfma(av[ks], w1, fe);
          ft = mfma(av[ks], w2, ft);
          ds = mfma(dv[ks], w0, ds);
          de = mfma(dv[ks], w1, de);
          dt = mfma(dv[ks], w2, dt);
        }
      }
      const float* hj = a.h + j * 3 * F + f;
      const float* xj = a.x + j * 3 * F + f;
      const float h_s = hj[0], h_e = hj[F], h_t = hj[2 * F], x0 = xj[0], x1 = xj[F], x2 = xj[2 * F];
      float c[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) c[q] = acc[(q * ncb + cb) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = grp * 4 + r;
        const int64_t i = ctr[row];
        const float gs = a.g_s[i * F + f];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (a.g_x) {
          const float* gx = a.g_x + i * 3 * F + f;
          g0 = gx[0];
          g1 = gx[F];
          g2 = gx[2 * F];
        }
        const float du = g0 * uvec[row * 4] + g1 * uvec[row * 4 + 1] + g2 * uvec[row * 4 + 2];
        const float dx = g0 * x0 + g1 * x1 + g2 * x2;
        c[0] += gs * fs[r];
        c[1] += du * fe[r];
        c[2] += dx * ft[r];
        const float gate = h_t * ft[r];
        c[3] += g0 * gate;
        c[4] += g1 * gate;
        c[5] += g2 * gate;
        gd[r] += gs * h_s * ds[r] + du * h_e * de[r] + dx * h_t * dt[r];
        const float ge = h_e * fe[r];
        gu0[r] += g0 * ge;
        gu1[r] += g1 * ge;
        gu2[r] += g2 * ge;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[(q * ncb + cb) * 64 + lane] = c[q];
    }
    // per-edge sums over the channels: the 16 lanes of a group, then the chain rule to the edge vector (u = r / d)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float vd = gd[r], v0 = gu0[r], v1 = gu1[r], v2 = gu2[r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        vd += __shfl_xor(vd, o, 64);
        v0 += __shfl_xor(v0, o, 64);
        v1 += __shfl_xor(v1, o, 64);
        v2 += __shfl_xor(v2, o, 64);
      }
      const int row = grp * 4 + r;
      const int e = eid[row];
      if (col == 0 && e >= 0) {
        const float ux = uvec[row * 4], uy = uvec[row * 4 + 1], uz = uvec[row * 4 + 2], inv_d = uvec[row * 4 + 3];
        const float gr = v0 * ux + v1 * uy + v2 * uz;
        const float gdd = inv_d > 0.f ? vd : 0.f;   // |r| has a zero subgradient at r = 0
        float o0 = gdd * ux + inv_d * (v0 - gr * ux), o1 = gdd * uy + inv_d * (v1 - gr * uy), o2 = gdd * uz + inv_d * (v2 - gr * uz);
        float* out = a.g_vec + (int64_t)e * 3;
        if (a.accumulate_vec) {
          o0 += out[0];
          o1 += out[1];
          o2 += out[2];
        }
        out[0] = o0;
        out[1] = o1;
        out[2] = o2;
      }
    }
  }
  for (int cb = 0; cb < ncb; ++cb) {
    const int f = cb * 16 + col;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      float v = acc[(q * ncb + cb) * 64 + lane];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (grp == 0) {
        if (q < 3) a.g_h[j * 3 * F + q * F + f] = v;
        else if (a.g_x_in) a.g_x_in[j * 3 * F + (q - 3) * F + f] = (a.g_x ? a.g_x[j * 3 * F + (q - 3) * F + f] : 0.f) + v;
      }
    }
  }
}

// ---- packed weights ----------------------------------------------------------------------------------------------------------------
// filter: out[k][n] = w[n][k] (k < B), b[n] (k = B), 0 behind            (w: rbf_lin.weight [3F, B])
__global__ void k_pack_filter(const float* w, const float* b, int F3, int B, float* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= KPAD * F3) return;
  const int k = t / F3, n = t - k * F3;
  out[t] = k < B ? w[(size_t)n * B + k] : (k == B ? b[n] : 0.f);
}
// update: four matrices in B-operand fragment order, out[((m ncb + cb) F / 4 + ks) 64 + lane] = W_m[k = 4 ks + (lane >> 4)][n = 16 cb + (lane & 15)],
// W_0[k][n] = U[n][k], W_1[k][n] = V[n][k] (forward: x W^T), W_2 = U, W_3 = V (reverse: g W)
__global__ void k_pack_uv(const float* wu, const float* wv, int F, float* out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)4 * F * F) return;
  const int lane = (int)(t & 63);
  int64_t q = t >> 6;
  const int ksn = F / 4, ncb = F / 16;
  const int ks = (int)(q % ksn);
  q /= ksn;
  const int cb = (int)(q % ncb), m = (int)(q / ncb);
  const int k = 4 * ks + (lane >> 4), n = 16 * cb + (lane & 15);
  const float* w = (m & 1) ? wv : wu;
  out[t] = m < 2 ? w[(size_t)n * F + k] : w[(size_t)k * F + n];
}

// ---- update block (painn.py:146-164) ------------------------------------------------------------------------------------------------
struct UpdArgs {
  int64_t n;
  int F;
  const float* s;
  const float* x;
  const float* wp;
  const float* a;       // update_mlp output [N, 3F]: a_ss | a_vv | a_sv
  float* U;             // [N, 3, F]
  float* V;
  float* ip;            // [N, F] <U, V>
  float* cat;           // [N, 2F] = [s | |V|]: the MLP's input
  const float* g_s;
  const float* g_x;     // may be null (zero)
  const float* g_cat;   // [N, 2F]
  float* g_s_in;
  float* g_x_in;
};

// one wave per (tile of 16 nodes, 16 output columns); the tile's three component planes are staged in LDS [3][TILE][F + 4]
__global__ void __launch_bounds__(256) k_update_uv_fwd(UpdArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, ld = F + 4, ncb = F >> 4, ksn = F >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * TILE;
  for (int q = threadIdx.x; q < 3 * TILE * F; q += blockDim.x) {
    const int k = q % F, c = (q / F) % 3, row = q / (3 * F);
    const int64_t n = n0 + row;
    lds[(c * TILE + row) * ld + k] = n < a.n ? a.x[n * 3 * F + c * F + k] : 0.f;
  }
  __syncthreads();
  const int cb = blockIdx.y * nw + wave;
  if (cb >= ncb) return;
  const int col = lane & 15, grp = lane >> 4;
  f32x4 u0 = {0.f, 0.f, 0.f, 0.f}, u1 = u0, u2 = u0, v0 = u0, v1 = u0, v2 = u0;
  const float* wu = a.wp + ((size_t)(0 * ncb + cb) * ksn) * 64 + lane;
  const float* wv = a.wp + ((size_t)(1 * ncb + cb) * ksn) * 64 + lane;
  const float* xa = lds + col * ld + grp;
#pragma unroll 4
  for (int ks = 0; ks < ksn; ++ks) {
    const float bu = wu[(size_t)ks * 64], bv = wv[(size_t)ks * 64];
    const float a0 = xa[ks * 4], a1 = xa[TILE * ld + ks * 4], a2 = xa[2 * TILE * ld + ks * 4];
    u0 = mfma(a0, bu, u0);
    u1 = mfma(a1, bu, u1);
    u2 = mfma(a2, bu, u2);
    v0 = mfma(a0, bv, v0);
    v1 = mfma(a1, bv, v1);
    v2 = mfma(a2, bv, v2);
  }
  const int f = cb * 16 + col;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t n = n0 + grp * 4 + r;
    if (n >= a.n) continue;
    float* Un = a.U + n * 3 * F + f;
    float* Vn = a.V + n * 3 * F + f;
    Un[0] = u0[r];
    Un[F] = u1[r];
    Un[2 * F] = u2[r];
    Vn[0] = v0[r];
    Vn[F] = v1[r];
    Vn[2 * F] = v2[r];
    a.ip[n * F + f] = u0[r] * v0[r] + u1[r] * v1[r] + u2[r] * v2[r];
    a.cat[n * 2 * F + f] = a.s[n * F + f];
    a.cat[n * 2 * F + F + f] = sqrtf(v0[r] * v0[r] + v1[r] * v1[r] + v2[r] * v2[r]);
  }
}

// s' = s + a_sv <U, V> + a_ss, x' = x + a_vv U (x_out null: nobody reads the vectors behind this block)
__global__ void k_update_out_fwd(int64_t n, int F, const float* s, const float* x, const float* a, const float* U, const float* ip, float* s_out,
                                 float* x_out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * F) return;
  const int64_t i = t / F;
  const int f = (int)(t - i * F);
  const float* ai = a + i * 3 * F + f;
  s_out[t] = s[t] + ai[2 * F] * ip[t] + ai[0];
  if (x_out) {
    const float avv = ai[F];
#pragma unroll
    for (int c = 0; c < 3; ++c) x_out[i * 3 * F + c * F + f] = x[i * 3 * F + c * F + f] + avv * U[i * 3 * F + c * F + f];
  }
}

// dL/da from dL/ds', dL/dx'
__global__ void k_update_out_bwd(int64_t n, int F, const float* g_s, const float* g_x, const float* U, const float* ip, float* g_a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * F) return;
  const int64_t i = t / F;
  const int f = (int)(t - i * F);
  const float gs = g_s[t];
  float gvv = 0.f;
  if (g_x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) gvv += g_x[i * 3 * F + c * F + f] * U[i * 3 * F + c * F + f];
  }
  float* ga = g_a + i * 3 * F + f;
  ga[0] = gs;
  ga[F] = gvv;
  ga[2 * F] = gs * ip[t];
}

// dL/dx = dL/dx' + dL/dU W_U + dL/dV W_V with dL/dU = a_vv dL/dx' + a_sv dL/ds' V, dL/dV = a_sv dL/ds' U + dL/d|V| V / |V|
// (zero where |V| = 0: torch's norm has a zero subgradient there); dL/ds = dL/ds' + dL/dcat[:, :F]
__global__ void __launch_bounds__(256) k_update_uv_bwd(UpdArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, ld = F + 4, ncb = F >> 4, ksn = F >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * TILE;
  const int cb = blockIdx.y * nw + wave;
  const int col = lane & 15, grp = lane >> 4;
  f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0, g2 = g0;
  for (int phase = 0; phase < 2; ++phase) {
    if (phase) __syncthreads();
    for (int q = threadIdx.x; q < 3 * TILE * F; q += blockDim.x) {
      const int k = q % F, c = (q / F) % 3, row = q / (3 * F);
      const int64_t n = n0 + row;
      float v = 0.f;
      if (n < a.n) {
        const int64_t o = n * 3 * F + c * F + k;
        const float gsv = a.a[n * 3 * F + 2 * F + k] * a.g_s[n * F + k];
        if (phase == 0) {
          v = gsv * a.V[o];
          if (a.g_x) v += a.a[n * 3 * F + F + k] * a.g_x[o];
        } else {
          const float vn = a.cat[n * 2 * F + F + k];
          v = gsv * a.U[o];
          if (vn > 0.f) v += a.g_cat[n * 2 * F + F + k] * a.V[o] / vn;
        }
      }
      lds[(c * TILE + row) * ld + k] = v;
    }
    __syncthreads();
    if (cb < ncb) {
      const float* w = a.wp + ((size_t)((2 + phase) * ncb + cb) * ksn) * 64 + lane;
      const float* xa = lds + col * ld + grp;
#pragma unroll 4
      for (int ks = 0; ks < ksn; ++ks) {
        const float b = w[(size_t)ks * 64];
        g0 = mfma(xa[ks * 4], b, g0);
        g1 = mfma(xa[TILE * ld + ks * 4], b, g1);
        g2 = mfma(xa[2 * TILE * ld + ks * 4], b, g2);
      }
    }
  }
  if (cb >= ncb) return;
  const int f = cb * 16 + col;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t n = n0 + grp * 4 + r;
    if (n >= a.n) continue;
    const int64_t o = n * 3 * F + f;
    a.g_x_in[o] = (a.g_x ? a.g_x[o] : 0.f) + g0[r];
    a.g_x_in[o + F] = (a.g_x ? a.g_x[o + F] : 0.f) + g1[r];
    a.g_x_in[o + 2 * F] = (a.g_x ? a.g_x[o + 2 * F] : 0.f) + g2[r];
    a.g_s_in[n * F + f] = a.g_s[n * F + f] + a.g_cat[n * 2 * F + f];
  }
}

__global__ void k_add(const float* a, const float* b, int64_t n, float* out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = a[t] + b[t];
}

static bool dims_ok(int node_dim, int num_basis) { return node_dim >= 32 && node_dim <= 256 && node_dim % 32 == 0 && num_basis >= 1 && num_basis <= KPAD - 1; }

// waves per workgroup and column split of the update products: few rows -> one wave per workgroup, a workgroup per 16 columns
static void uv_shape(int64_t n, int F, dim3& grid, dim3& block) {
  const int ncb = F / 16;
  const int nw = n <= FEW_ROWS ? 1 : (ncb % 4 == 0 ? 4 : 2);
  grid = dim3((unsigned)((n + TILE - 1) / TILE), (unsigned)(ncb / nw));
  block = dim3(64 * nw);
}

}  // namespace painn
}  // namespace xeq

using namespace xeq;
using namespace xeq::painn;

extern "C" {

int xeq_painn_supported(int dtype, int node_dim, int num_basis) { return dtype == XEQ_F32 && dims_ok(node_dim, num_basis) ? 1 : 0; }

int64_t xeq_painn_few_rows_limit(void) { return FEW_ROWS; }

int64_t xeq_painn_filter_packed_floats(int node_dim) { return (int64_t)KPAD * 3 * node_dim; }

int64_t xeq_painn_uv_packed_floats(int node_dim) { return (int64_t)4 * node_dim * node_dim; }

int xeq_painn_pack_filter(const float* w, const float* b, int node_dim, int num_basis, float* out, void* stream) {
  XEQ_CHECK_ARG(w && b && out, "xeq_painn_pack_filter: null buffer");
  XEQ_CHECK_ARG(dims_ok(node_dim, num_basis), "xeq_painn_pack_filter: node_dim %d / num_basis %d not supported", node_dim, num_basis);
  const int total = KPAD * 3 * node_dim;
  hipLaunchKernelGGL(k_pack_filter, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, b, 3 * node_dim, num_basis, out);
  XEQ_CHECK_LAUNCH("xeq_painn_pack_filter");
  return XEQ_OK;
}

int xeq_painn_pack_uv(const float* wu, const float* wv, int node_dim, float* out, void* stream) {
  XEQ_CHECK_ARG(wu && wv && out, "xeq_painn_pack_uv: null buffer");
  XEQ_CHECK_ARG(dims_ok(node_dim, 1), "xeq_painn_pack_uv: node_dim %d not supported", node_dim);
  const int64_t total = (int64_t)4 * node_dim * node_dim;
  hipLaunchKernelGGL(k_pack_uv, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wu, wv, node_dim, out);
  XEQ_CHECK_LAUNCH("xeq_painn_pack_uv");
  return XEQ_OK;
}

int xeq_painn_message_fwd(int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* perm, const int64_t* edge_index, const float* vec,
                          const float* h, const float* s, const float* x, const float* wp, const float* p0, const float* p1, int rbf_kind,
                          int cutoff_kind, int num_basis, double cutoff, int node_dim, float* s_out, float* x_out, void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, num_basis), "xeq_painn_message_fwd: node_dim %d / num_basis %d not supported", node_dim, num_basis);
  XEQ_CHECK_ARG(n_nodes >= 0 && n_edges >= 0, "xeq_painn_message_fwd: negative size");
  if (n_nodes == 0) return XEQ_OK;
  XEQ_CHECK_ARG(rowptr && h && s && x && wp && p0 && s_out && x_out && (n_edges == 0 || (edge_index && vec)), "xeq_painn_message_fwd: null buffer");
  MsgArgs a{};
  a.n_nodes = n_nodes; a.n_edges = n_edges; a.rowptr = rowptr; a.perm = perm; a.edge_index = edge_index; a.vec = vec; a.h = h; a.s = s; a.x = x;
  a.wp = wp; a.p0 = p0; a.p1 = p1; a.rbf_kind = rbf_kind; a.cutoff_kind = cutoff_kind; a.num_basis = num_basis; a.cutoff = (float)cutoff;
  a.F = node_dim; a.s_out = s_out; a.x_out = x_out;
  const int nw = node_dim <= 128 ? 4 : 2;
  const size_t per_wave = sizeof(float) * (CHUNK * BROW + CHUNK * 4 + CHUNK + 4 * (node_dim / 16) * 64);
  hipLaunchKernelGGL(k_message_fwd, dim3((unsigned)((n_nodes + nw - 1) / nw)), dim3(64 * nw), nw * per_wave, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_painn_message_fwd");
  return XEQ_OK;
}

int xeq_painn_message_bwd(int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm, const int64_t* edge_index, const float* vec,
                          const float* h, const float* x, const float* wp, const float* p0, const float* p1, int rbf_kind, int cutoff_kind,
                          int num_basis, double cutoff, int node_dim, const float* g_s, const float* g_x, float* g_h, float* g_x_in, float* g_vec,
                          int accumulate_vec, void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, num_basis), "xeq_painn_message_bwd: node_dim %d / num_basis %d not supported", node_dim, num_basis);
  XEQ_CHECK_ARG(n_nodes >= 0 && n_edges >= 0, "xeq_painn_message_bwd: negative size");
  if (n_nodes == 0) return XEQ_OK;
  XEQ_CHECK_ARG(n_rowptr && h && x && wp && p0 && g_s && g_h && (n_edges == 0 || (edge_index && vec && g_vec)), "xeq_painn_message_bwd: null buffer");
  MsgArgs a{};
  a.n_nodes = n_nodes; a.n_edges = n_edges; a.rowptr = n_rowptr; a.perm = n_perm; a.edge_index = edge_index; a.vec = vec; a.h = h; a.x = x;
  a.wp = wp; a.p0 = p0; a.p1 = p1; a.rbf_kind = rbf_kind; a.cutoff_kind = cutoff_kind; a.num_basis = num_basis; a.cutoff = (float)cutoff;
  a.F = node_dim; a.g_s = g_s; a.g_x = g_x; a.g_h = g_h; a.g_x_in = g_x_in; a.g_vec = g_vec; a.accumulate_vec = accumulate_vec;
  const int nw = node_dim <= 128 ? 2 : 1;
  const size_t per_wave = sizeof(float) * (2 * CHUNK * BROW + CHUNK * 4 + 2 * CHUNK + 6 * (node_dim / 16) * 64);
  hipLaunchKernelGGL(k_message_bwd, dim3((unsigned)((n_nodes + nw - 1) / nw)), dim3(64 * nw), nw * per_wave, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_painn_message_bwd");
  return XEQ_OK;
}

int xeq_painn_update_uv_fwd(int64_t n, int node_dim, const float* s, const float* x, const float* wp, float* U, float* V, float* ip, float* cat,
                            void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, 1) && n >= 0, "xeq_painn_update_uv_fwd: node_dim %d not supported", node_dim);
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(s && x && wp && U && V && ip && cat, "xeq_painn_update_uv_fwd: null buffer");
  UpdArgs a{};
  a.n = n; a.F = node_dim; a.s = s; a.x = x; a.wp = wp; a.U = U; a.V = V; a.ip = ip; a.cat = cat;
  dim3 grid, block;
  uv_shape(n, node_dim, grid, block);
  hipLaunchKernelGGL(k_update_uv_fwd, grid, block, sizeof(float) * 3 * TILE * (node_dim + 4), (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_painn_update_uv_fwd");
  return XEQ_OK;
}

int xeq_painn_update_out_fwd(int64_t n, int node_dim, const float* s, const float* x, const float* a, const float* U, const float* ip, float* s_out,
                             float* x_out, void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, 1) && n >= 0, "xeq_painn_update_out_fwd: node_dim %d not supported", node_dim);
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(s && a && ip && s_out && (!x_out || (x && U)), "xeq_painn_update_out_fwd: null buffer");
  const int64_t total = n * node_dim;
  hipLaunchKernelGGL(k_update_out_fwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, node_dim, s, x, a, U, ip, s_out, x_out);
  XEQ_CHECK_LAUNCH("xeq_painn_update_out_fwd");
  return XEQ_OK;
}

int xeq_painn_update_out_bwd(int64_t n, int node_dim, const float* g_s, const float* g_x, const float* U, const float* ip, float* g_a, void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, 1) && n >= 0, "xeq_painn_update_out_bwd: node_dim %d not supported", node_dim);
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(g_s && U && ip && g_a, "xeq_painn_update_out_bwd: null buffer");
  const int64_t total = n * node_dim;
  hipLaunchKernelGGL(k_update_out_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, node_dim, g_s, g_x, U, ip, g_a);
  XEQ_CHECK_LAUNCH("xeq_painn_update_out_bwd");
  return XEQ_OK;
}

int xeq_painn_update_uv_bwd(int64_t n, int node_dim, const float* g_s, const float* g_x, const float* a, const float* U, const float* V, const float* cat,
                            const float* g_cat, const float* wp, float* g_s_in, float* g_x_in, void* stream) {
  XEQ_CHECK_ARG(dims_ok(node_dim, 1) && n >= 0, "xeq_painn_update_uv_bwd: node_dim %d not supported", node_dim);
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(g_s && a && U && V && cat && g_cat && wp && g_s_in && g_x_in, "xeq_painn_update_uv_bwd: null buffer");
  UpdArgs u{};
  u.n = n; u.F = node_dim; u.g_s = g_s; u.g_x = g_x; u.a = a; u.U = const_cast<float*>(U); u.V = const_cast<float*>(V); u.cat = const_cast<float*>(cat); u.g_cat = g_cat; u.wp = wp; u.g_s_in = g_s_in; u.g_x_in = g_x_in;
  dim3 grid, block;
  uv_shape(n, node_dim, grid, block);
  hipLaunchKernelGGL(k_update_uv_bwd, grid, block, sizeof(float) * 3 * TILE * (node_dim + 4), (hipStream_t)stream, u);
  XEQ_CHECK_LAUNCH("xeq_painn_update_uv_bwd");
  return XEQ_OK;
}

int xeq_painn_add(const float* a, const float* b, int64_t n, float* out, void* stream) {
  XEQ_CHECK_ARG(n >= 0, "xeq_painn_add: negative size");
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(a && b && out, "xeq_painn_add: null buffer");
  hipLaunchKernelGGL(k_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, out);
  XEQ_CHECK_LAUNCH("xeq_painn_add");
  return XEQ_OK;
}

}  // extern "C"
