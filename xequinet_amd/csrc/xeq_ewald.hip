// Ewald message passing (reference nn/ewald.py:141-212 EwaldBlock with the geometry of :60-138), f32 inference with an explicit reverse
// pass.  Atom n of graph g at pos_n, k-vectors kvec[g, k, :] (graph stride 0: one table for every graph), theta_nk = <kvec[g, k], pos_n>,
// damping d_n (NULL: 1), rows x [n, F], filter kf [K, F]:
//   k_ewald_sf      S_R[g, k, f] = sum_{n in g} d_n cos(theta_nk) x[n, f],  S_I the same with sin          (xeq_ewald_structure_factor)
//   k_ewald_apply   m[n, f] = d_n sum_k kf[k, f] (cos(theta_nk) S_R[g, k, f] + sin(theta_nk) S_I[g, k, f])  (xeq_ewald_apply)
//   k_ewald_phase   T1[n, k] = sum_f kf[k, f] (gm[n, f] S_R[g, k, f] + h[n, f] P_R[g, k, f]), T2 with the imaginary parts,
//                   dL/dtheta_nk = d_n (-sin T1 + cos T2), dL/dd_n = sum_k (cos T1 + sin T2),
//                   dL/dpos_n = sum_k dL/dtheta_nk kvec[g, k] + dL/dd_n dd_n/dpos_n                          (xeq_ewald_phase_grad)
// Design.  A graph is cut into chunks of EW_CHUNK = 64 atoms counted from its first atom; workgroup b (4 waves) finds its (graph, chunk)
// in `ptr` by binary search over the slot bases ptr[g] / 64 + g (strictly increasing, at least as many slots between two bases as the
// graph has chunks, n / 64 + G slots in all, so the grid needs no count read back from the device).  Phases are computed in the kernels
// from pos and kvec, in f32 with one fixed fma order and the accurate sincosf, staged in LDS and contracted on the exact-f32 matrix
// instruction v_mfma_f32_32x32x2_f32 (conventions of xeq_electronic.hip / xeq_heads.hip): over a chunk's atoms for S (output tile 32 k x
// 32 f), over k for m (32 atoms x 32 f), over f for T1 / T2 (32 k x 32 atoms, so that an atom's sum over k stays inside a lane).  K is
// padded to the tile of 32 inside the kernels with zero rows.
// Determinism: no float atomics.  A graph of one chunk writes S itself; a larger one writes a partial per chunk and k_ewald_sf_sum adds
// them in chunk order.  Every sum's order depends on the graph's own atom count alone, so a graph's S, m and gradients are bit-identical
// alone, inside any batch, in a shard and on repeat.
// Row kernels of the block's glue: LayerNorm over F forward / reverse (one wave per row, a fixed butterfly), (sa a + sb b) [silu'(pre)],
// and the damping prod_i sinc(a pos_i + eps) with its position derivative.
#include "xeq_common.h"
#include "xeq_linear_s.h"

namespace xeq {

constexpr int EW_CHUNK = 64;      // atoms per chunk (two 32-row tiles)
constexpr int EW_KMAX = 192;      // k-points (six tiles of 32); the reference's periodic default [3, 3, 3] has 171
constexpr int EW_FS = 32;         // f-slab of the phase-gradient contraction
constexpr int EW_FLD = EW_FS + 1; // odd LDS row stride: the operands are read down a column

struct EwGeom {
  const float* pos;      // [n, 3]
  const float* kvec;     // [G or 1, K, 3]
  int64_t kstride;       // floats between two graphs' tables (0: shared)
  const float* damp;     // [n] or NULL
  const int64_t* ptr;    // [G + 1]
  int64_t G, n;
  int K, F;
};

// (graph, first atom, atoms, chunk index, chunks of the graph) of slot b; false: the slot is unused
__device__ __forceinline__ bool ew_slot(const EwGeom& e, int64_t b, int64_t& g, int64_t& a0, int& rows, int& chunk, int& nch) {
  int64_t lo = 0, hi = e.G;   // last g with ptr[g] / 64 + g <= b
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (e.ptr[mid] / EW_CHUNK + mid <= b) lo = mid;
    else hi = mid;
  }
  g = lo;
  const int64_t first = max((int64_t)0, min(e.ptr[g], e.n)), last = max(first, min(e.ptr[g + 1], e.n));
  const int64_t cnt = last - first, j = b - (e.ptr[g] / EW_CHUNK + g);
  nch = (int)((cnt + EW_CHUNK - 1) / EW_CHUNK);
  if (j < 0 || j >= max(nch, 1)) return false;   // chunk 0 of an empty graph still runs: it writes the zeros
  chunk = (int)j;
  a0 = first + j * EW_CHUNK;
  rows = (int)min((int64_t)EW_CHUNK, cnt - j * EW_CHUNK);
  return true;
}

__device__ __forceinline__ float ew_theta(const float* __restrict__ kv, float px, float py, float pz) {
  return fmaf(kv[2], pz, fmaf(kv[1], py, kv[0] * px));
}

// d cos(theta), d sin(theta) of the chunk's atoms and the 32 k-points of tile kt into Tc / Ts [atom][ld] (zeros past rows / K)
__device__ __forceinline__ void ew_stage_trig(const EwGeom& e, int64_t g, int64_t a0, int rows, int kt, float* Tc, float* Ts, int ld) {
  for (int idx = threadIdx.x; idx < EW_CHUNK * 32; idx += 256) {
    const int atom = idx >> 5, kl = idx & 31, k = 32 * kt + kl;
    float c = 0.f, s = 0.f;
    if (atom < rows && k < e.K) {
      const float* p = e.pos + (a0 + atom) * 3;
      const float th = ew_theta(e.kvec + g * e.kstride + 3 * k, p[0], p[1], p[2]);
      sincosf(th, &s, &c);
      const float d = e.damp ? e.damp[a0 + atom] : 1.f;
      c *= d;
      s *= d;
    }
    Tc[atom * ld + kl] = c;
    Ts[atom * ld + kl] = s;
  }
}

// ---- structure factor ------------------------------------------------------------------------------------------------------------
struct SfArgs {
  EwGeom e;
  const float* X;     // [n, ldx]
  int64_t ldx;
  float* parts;       // [slots, 2, K, F]
  float* SR;          // [G, K, F]
  float* SI;
};

__global__ void __launch_bounds__(256) k_ewald_sf(SfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ew_lds[];
  const EwGeom& e = a.e;
  float* Tc = ew_lds;                    // [64][32]
  float* Ts = Tc + EW_CHUNK * 32;        // [64][32]
  float* Hs = Ts + EW_CHUNK * 32;        // [64][F]
  int64_t g, a0;
  int rows, chunk, nch;
  if (!ew_slot(e, blockIdx.x, g, a0, rows, chunk, nch)) return;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, kh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.y, F = e.F;
  ew_stage_trig(e, g, a0, rows, kt, Tc, Ts, 32);
  const int f4 = F >> 2;
  for (int idx = tid; idx < EW_CHUNK * f4; idx += 256) {
    const int r = idx / f4, c4 = idx - r * f4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = *reinterpret_cast<const float4*>(a.X + (a0 + r) * a.ldx + 4 * c4);
    *reinterpret_cast<float4*>(&Hs[r * F + 4 * c4]) = v;
  }
  __syncthreads();
  const int nq = (rows + 1) >> 1, FT = F >> 5;
  for (int job = wave; job < 2 * FT; job += 4) {
    const int ft = job >> 1, ri = job & 1;
    const float* T = ri ? Ts : Tc;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int q = 0; q < nq; ++q)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(T[(2 * q + kh) * 32 + i], Hs[(2 * q + kh) * F + 32 * ft + i], acc, 0, 0, 0);
    float* dst = nch <= 1 ? (ri ? a.SI : a.SR) + g * (int64_t)e.K * F : a.parts + ((int64_t)blockIdx.x * 2 + ri) * e.K * F;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (k < e.K) dst[(int64_t)k * F + 32 * ft + i] = acc[r];
    }
  }
}

// S[g] = sum of the graph's chunk partials in chunk order (graphs of more than one chunk)
__global__ void __launch_bounds__(256) k_ewald_sf_sum(SfArgs a) {
  const EwGeom& e = a.e;
  const int64_t g = blockIdx.x;
  const int64_t first = max((int64_t)0, min(e.ptr[g], e.n)), last = max(first, min(e.ptr[g + 1], e.n));
  const int nch = (int)((last - first + EW_CHUNK - 1) / EW_CHUNK);
  if (nch <= 1) return;
  const int64_t base = e.ptr[g] / EW_CHUNK + g, KF = (int64_t)e.K * e.F;
  for (int64_t idx = (int64_t)blockIdx.y * 256 + threadIdx.x; idx < 2 * KF; idx += (int64_t)gridDim.y * 256) {
    float acc = a.parts[base * 2 * KF + idx];
    for (int j = 1; j < nch; ++j) acc += a.parts[(base + j) * 2 * KF + idx];
    if (idx < KF) a.SR[g * KF + idx] = acc;
    else a.SI[g * KF + idx - KF] = acc;
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
struct ApArgs {
  EwGeom e;
  const float* SR;    // [G, K, F]
  const float* SI;
  const float* kf;    // [K, F]
  float* out;         // [n, ldo]
  int64_t ldo;
};

__global__ void __launch_bounds__(256) k_ewald_apply(ApArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ew_lds[];
  const EwGeom& e = a.e;
  float* Tc = ew_lds;                    // [64][33]
  float* Ts = Tc + EW_CHUNK * 33;        // [64][33]
  float* WR = Ts + EW_CHUNK * 33;        // [32][F]  kf S_R of this k-tile
  float* WI = WR + 32 * e.F;             // [32][F]
  int64_t g, a0;
  int rows, chunk, nch;
  if (!ew_slot(e, blockIdx.x, g, a0, rows, chunk, nch) || rows == 0) return;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, kh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = e.F, FT = F >> 5, KT = (e.K + 31) >> 5;
  const int at = wave & 1, ft0 = wave >> 1;
  const bool active = 32 * at < rows;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int kt = 0; kt < KT; ++kt) {
    __syncthreads();
    ew_stage_trig(e, g, a0, rows, kt, Tc, Ts, 33);
    for (int idx = tid; idx < 32 * F; idx += 256) {
      const int kl = idx / F, f = idx - kl * F, k = 32 * kt + kl;
      float wr = 0.f, wi = 0.f;
      if (k < e.K) {
        const float w = a.kf[(int64_t)k * F + f];
        const int64_t at_s = (g * e.K + k) * F + f;
        wr = w * a.SR[at_s];
        wi = w * a.SI[at_s];
      }
      WR[idx] = wr;
      WI[idx] = wi;
    }
    __syncthreads();
    if (active) {
      const int nq = min(16, (e.K - 32 * kt + 1) >> 1);
      // a fresh chain per k-tile (64 terms), added to the running sum: the rounding error grows with the tile count, not with 2 K
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ft = ft0 + 2 * j;
        if (ft >= FT) continue;
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = 0.f;
        for (int q = 0; q < nq; ++q) {
          const int k = 2 * q + kh;
          t = __builtin_amdgcn_mfma_f32_32x32x2f32(Tc[(32 * at + i) * 33 + k], WR[k * F + 32 * ft + i], t, 0, 0, 0);
          t = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[(32 * at + i) * 33 + k], WI[k * F + 32 * ft + i], t, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] += t[r];
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ft = ft0 + 2 * j;
    if (ft >= FT) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * at + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (row < rows) a.out[(a0 + row) * a.ldo + 32 * ft + i] = acc[j][r];
    }
  }
}

// ---- phase gradient ----------------------------------------------------------------------------------------------------------------
struct EwPhaseArgs {
  EwGeom e;
  const float* GM;    // [n, ldg] dL/dm
  const float* H;     // [n, ldh]
  int64_t ldg, ldh;
  const float* SR;    // structure factors of h
  const float* SI;
  const float* PR;    // structure factors of gm
  const float* PI;
  const float* kf;
  const float* ddamp; // [n, 3] or NULL
  float* g_theta;     // [n, K] or NULL
  float* g_damp;      // [n] or NULL
  float* g_pos;       // [n, 3]
};

__global__ void __launch_bounds__(256) k_ewald_phase(EwPhaseArgs a) {
  // W[kk][which][32][33]: the four filtered structure factors (S_R, S_I, P_R, P_I) of the two k-tiles in flight; R[2][64][33]: gm, h
  __shared__ float W[2][4][32 * EW_FLD];
  __shared__ float R[2][EW_CHUNK * EW_FLD];
  __shared__ float red[2][32][4];
  const EwGeom& e = a.e;
  int64_t g, a0;
  int rows, chunk, nch;
  if (!ew_slot(e, blockIdx.x, g, a0, rows, chunk, nch) || rows == 0) return;
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, kh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = e.F, K = e.K, KT = (K + 31) >> 5;
  const int at = wave & 1, kk = wave >> 1;
  const int my = 32 * at + i;
  const bool mine = my < rows;
  float px = 0.f, py = 0.f, pz = 0.f, d = 1.f;
  if (mine) {
    const float* p = e.pos + (a0 + my) * 3;
    px = p[0];
    py = p[1];
    pz = p[2];
    if (e.damp) d = e.damp[a0 + my];
  }
  float gx = 0.f, gy = 0.f, gz = 0.f, gd = 0.f;
  const float* const src[4] = {a.SR, a.SI, a.PR, a.PI};
  for (int kt0 = 0; kt0 < KT; kt0 += 2) {
    const int kt = kt0 + kk;
    const bool active = kt < KT && 32 * at < rows;
    f32x16 t1, t2;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1[r] = t2[r] = 0.f;
    for (int f0 = 0; f0 < F; f0 += EW_FS) {
      __syncthreads();
      for (int idx = tid; idx < 2 * 32 * EW_FS; idx += 256) {
        const int t = idx / (32 * EW_FS), rem = idx - t * 32 * EW_FS, kl = rem / EW_FS, fl = rem - kl * EW_FS;
        const int k = 32 * (kt0 + t) + kl, f = f0 + fl;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (k < K) {
          const float w = a.kf[(int64_t)k * F + f];
          const int64_t at_s = (g * K + k) * F + f;
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = w * src[c][at_s];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) W[t][c][kl * EW_FLD + fl] = v[c];
      }
      for (int idx = tid; idx < EW_CHUNK * EW_FS; idx += 256) {
        const int r = idx / EW_FS, fl = idx - r * EW_FS;
        float vg = 0.f, vh = 0.f;
        if (r < rows) {
          vg = a.GM[(a0 + r) * a.ldg + f0 + fl];
          vh = a.H[(a0 + r) * a.ldh + f0 + fl];
        }
        R[0][r * EW_FLD + fl] = vg;
        R[1][r * EW_FLD + fl] = vh;
      }
      __syncthreads();
      if (active) {
        // four fresh chains of 32 terms per slab (gm S_R, gm S_I, h P_R, h P_I), added to the running sums: the rounding error
        // grows with the slab count, not with 2 F
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f32x16 t;
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = 0.f;
          for (int q = 0; q < EW_FS / 2; ++q) {
            const int f = 2 * q + kh;
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(W[kk][c][i * EW_FLD + f], R[c >> 1][my * EW_FLD + f], t, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (c & 1) t2[r] += t[r];
            else t1[r] += t[r];
          }
        }
      }
    }
    if (active && mine) {   // this lane: atom `my`, the 16 k-points (r & 3) + 8 (r >> 2) + 4 kh of tile kt
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (k < K) {
          const float* kv = e.kvec + g * e.kstride + 3 * k;
          float s, c;
          sincosf(ew_theta(kv, px, py, pz), &s, &c);
          const float gt = d * (c * t2[r] - s * t1[r]);
          gd += c * t1[r] + s * t2[r];
          gx = fmaf(gt, kv[0], gx);
          gy = fmaf(gt, kv[1], gy);
          gz = fmaf(gt, kv[2], gz);
          if (a.g_theta) a.g_theta[(a0 + my) * K + k] = gt;
        }
      }
    }
  }
  // the two lane halves (k rows 4 kh), then the two k-tile parities, in one fixed order
  gx += __shfl_xor(gx, 32, 64);
  gy += __shfl_xor(gy, 32, 64);
  gz += __shfl_xor(gz, 32, 64);
  gd += __shfl_xor(gd, 32, 64);
  __syncthreads();
  if (kk == 1 && kh == 0) {
    red[at][i][0] = gx;
    red[at][i][1] = gy;
    red[at][i][2] = gz;
    red[at][i][3] = gd;
  }
  __syncthreads();
  if (kk == 0 && kh == 0 && mine) {
    gx += red[at][i][0];
    gy += red[at][i][1];
    gz += red[at][i][2];
    gd += red[at][i][3];
    const int64_t n = a0 + my;
    if (a.ddamp) {
      gx = fmaf(gd, a.ddamp[n * 3], gx);
      gy = fmaf(gd, a.ddamp[n * 3 + 1], gy);
      gz = fmaf(gd, a.ddamp[n * 3 + 2], gz);
    }
    a.g_pos[n * 3] = gx;
    a.g_pos[n * 3 + 1] = gy;
    a.g_pos[n * 3 + 2] = gz;
    if (a.g_damp) a.g_damp[n] = gd;
  }
}

// ---- row kernels -------------------------------------------------------------------------------------------------------------------
// sinc(x) = sin(pi x) / (pi x) (torch.sinc) and its derivative; the series below |pi x| = 0.5 (the closed form cancels there)
__device__ __forceinline__ void ew_sinc(float x, float& v, float& dv) {
  const float PI = 3.14159265358979323846f;
  const float t = PI * x;
  if (fabsf(t) < 0.5f) {
    const float t2 = t * t;
    v = 1.f + t2 * (-1.f / 6.f + t2 * (1.f / 120.f + t2 * (-1.f / 5040.f + t2 * (1.f / 362880.f))));
    dv = PI * t * (-1.f / 3.f + t2 * (1.f / 30.f + t2 * (-1.f / 840.f + t2 * (1.f / 45360.f))));
  } else {
    float s, c;
    sincosf(t, &s, &c);
    v = s / t;
    dv = (c - v) / x;
  }
}

__global__ void __launch_bounds__(256) k_ewald_damping(const float* __restrict__ pos, int64_t n, float scale, float eps, float* __restrict__ damp,
                                                       float* __restrict__ ddamp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float v[3], dv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) ew_sinc(fmaf(scale, pos[idx * 3 + c], eps), v[c], dv[c]);
  damp[idx] = (v[0] * v[1]) * v[2];
  if (ddamp) {
    ddamp[idx * 3] = scale * dv[0] * (v[1] * v[2]);
    ddamp[idx * 3 + 1] = scale * dv[1] * (v[0] * v[2]);
    ddamp[idx * 3 + 2] = scale * dv[2] * (v[0] * v[1]);
  }
}

// LayerNorm over F (<= 256): one wave per row, lane l holds the columns l, l + 64, ...; stats[row] = (mean, rstd)
__global__ void __launch_bounds__(256) k_ewald_ln_fwd(const float* __restrict__ x, int64_t n, int F, const float* __restrict__ w,
                                                      const float* __restrict__ b, float eps, float* __restrict__ y, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float v[4], sum = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    v[c] = col < F ? x[row * F + col] : 0.f;
    sum += v[c];
  }
  const float mean = wave_sum(sum) / (float)F;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float dlt = lane + 64 * c < F ? v[c] - mean : 0.f;
    sq = fmaf(dlt, dlt, sq);
  }
  const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)F + eps);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    if (col < F) y[row * F + col] = fmaf((v[c] - mean) * rstd, w[col], b[col]);
  }
  if (lane == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = rstd;
  }
}

// g_x = rstd (g w - mean(g w) - xhat mean(g w xhat))
__global__ void __launch_bounds__(256) k_ewald_ln_bwd(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ stats,
                                                      const float* __restrict__ w, int64_t n, int F, float* __restrict__ gx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
  float gw[4], xh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    gw[c] = col < F ? g[row * F + col] * w[col] : 0.f;
    xh[c] = col < F ? (x[row * F + col] - mean) * rstd : 0.f;
    s1 += gw[c];
    s2 = fmaf(gw[c], xh[c], s2);
  }
  const float m1 = wave_sum(s1) / (float)F, m2 = wave_sum(s2) / (float)F;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    if (col < F) gx[row * F + col] = rstd * (gw[c] - m1 - xh[c] * m2);
  }
}

// out = (sa a + sb b) [silu'(pre)]
__global__ void __launch_bounds__(256) k_ewald_combine(const float* __restrict__ a, float sa, const float* __restrict__ b, float sb,
                                                       const float* __restrict__ pre, int64_t count, float* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (int64_t)gridDim.x * 256) {
    float v = sa * a[idx];
    if (b) v = fmaf(sb, b[idx], v);
    if (pre) {
      v *= silu_grad_f(pre[idx]);
    }
    out[idx] = v;
  }
}

}  // namespace xeq

using namespace xeq;

static bool ew_shape_ok(int node_dim, int n_k) { return node_dim >= 32 && node_dim <= 256 && node_dim % 32 == 0 && n_k >= 1 && n_k <= EW_KMAX; }
static size_t ew_sf_lds(int F) { return sizeof(float) * (size_t)(2 * EW_CHUNK * 32 + EW_CHUNK * F); }
static size_t ew_apply_lds(int F) { return sizeof(float) * (size_t)(2 * EW_CHUNK * 33 + 2 * 32 * F); }

// dynamic LDS above the default 64 KB at node_dim 256
static hipError_t ew_raise_lds() {
  static const hipError_t r1 = raise_dynamic_lds({reinterpret_cast<const void*>(&k_ewald_sf)}, ew_sf_lds(256));
  static const hipError_t r2 = raise_dynamic_lds({reinterpret_cast<const void*>(&k_ewald_apply)}, ew_apply_lds(256));
  return r1 != hipSuccess ? r1 : r2;
}

static int ew_geom(const char* who, EwGeom& e, const void* pos, const void* kvec, int64_t kvec_gstride, int n_k, const void* damp, const int64_t* ptr,
                   int64_t n_graphs, int64_t n, int node_dim) {
  XEQ_CHECK_ARG(n >= 0 && n_graphs >= 0 && ew_shape_ok(node_dim, n_k), "%s: node_dim %d (multiples of 32, <= 256), %d k-points (1 .. %d)", who, node_dim,
                n_k, EW_KMAX);
  XEQ_CHECK_ARG(kvec_gstride == 0 || kvec_gstride >= (int64_t)3 * n_k, "%s: graph stride %lld of the k-vector table", who, (long long)kvec_gstride);
  XEQ_CHECK_ARG(n_graphs == 0 || (ptr && kvec && (n == 0 || pos)), "%s: null buffer", who);
  e = EwGeom{(const float*)pos, (const float*)kvec, kvec_gstride, (const float*)damp, ptr, n_graphs, n, n_k, node_dim};
  return XEQ_OK;
}

extern "C" {

int xeq_ewald_supported(int dtype, int node_dim, int n_k) { return dtype == XEQ_F32 && ew_shape_ok(node_dim, n_k) ? 1 : 0; }

int64_t xeq_ewald_chunk(void) { return EW_CHUNK; }

// The host knows n and G but not the largest graph (that count lives on the device and is not read back): above one chunk of atoms in
// all, the workspace has a partial per slot and k_ewald_sf_sum is launched for every graph; where no graph exceeds a chunk its
// workgroups return at once and the partials stay unused (QM9-1024 at K = 13, F = 128: 17 MB reserved, one idle launch).
int64_t xeq_ewald_parts_floats(int64_t n, int64_t n_graphs, int n_k, int node_dim) {
  return n <= EW_CHUNK ? 0 : (n / EW_CHUNK + n_graphs) * 2 * (int64_t)n_k * node_dim;
}

int xeq_ewald_structure_factor(const void* x, int64_t ldx, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride, int n_k,
                               const void* damp, const int64_t* ptr, int64_t n_graphs, void* parts, void* s_r, void* s_i, void* stream) {
  SfArgs a{};
  const int st = ew_geom("xeq_ewald_structure_factor", a.e, pos, kvec, kvec_gstride, n_k, damp, ptr, n_graphs, n, node_dim);
  if (st != XEQ_OK) return st;
  XEQ_CHECK_ARG(ldx >= node_dim && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, "xeq_ewald_structure_factor: row stride %lld / alignment of x", (long long)ldx);
  XEQ_CHECK_ARG(n_graphs == 0 || (s_r && s_i && (n == 0 || x) && (n <= EW_CHUNK || parts)), "xeq_ewald_structure_factor: null buffer");
  if (n_graphs == 0) return XEQ_OK;
  XEQ_CHECK_ARG(ew_raise_lds() == hipSuccess, "xeq_ewald_structure_factor: cannot raise the dynamic LDS limit");
  a.X = (const float*)x;
  a.ldx = ldx;
  a.parts = (float*)parts;
  a.SR = (float*)s_r;
  a.SI = (float*)s_i;
  const unsigned slots = (unsigned)(n / EW_CHUNK + n_graphs), KT = (unsigned)((n_k + 31) / 32);
  hipLaunchKernelGGL(k_ewald_sf, dim3(slots, KT), dim3(256), ew_sf_lds(node_dim), (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_ewald_structure_factor");
  if (n > EW_CHUNK) {   // only then can a graph have more than one chunk
    hipLaunchKernelGGL(k_ewald_sf_sum, dim3((unsigned)n_graphs, 8), dim3(256), 0, (hipStream_t)stream, a);
    XEQ_CHECK_LAUNCH("xeq_ewald_structure_factor_sum");
  }
  return XEQ_OK;
}

int xeq_ewald_apply(const void* s_r, const void* s_i, const void* kf, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride,
                    int n_k, const void* damp, const int64_t* ptr, int64_t n_graphs, void* out, int64_t ldo, void* stream) {
  ApArgs a{};
  const int st = ew_geom("xeq_ewald_apply", a.e, pos, kvec, kvec_gstride, n_k, damp, ptr, n_graphs, n, node_dim);
  if (st != XEQ_OK) return st;
  XEQ_CHECK_ARG(ldo >= node_dim, "xeq_ewald_apply: row stride %lld of out", (long long)ldo);
  XEQ_CHECK_ARG(n == 0 || (s_r && s_i && kf && out && n_graphs >= 1), "xeq_ewald_apply: null buffer or no graph");
  if (n == 0) return XEQ_OK;
  XEQ_CHECK_ARG(ew_raise_lds() == hipSuccess, "xeq_ewald_apply: cannot raise the dynamic LDS limit");
  a.SR = (const float*)s_r;
  a.SI = (const float*)s_i;
  a.kf = (const float*)kf;
  a.out = (float*)out;
  a.ldo = ldo;
  hipLaunchKernelGGL(k_ewald_apply, dim3((unsigned)(n / EW_CHUNK + n_graphs)), dim3(256), ew_apply_lds(node_dim), (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_ewald_apply");
  return XEQ_OK;
}

int xeq_ewald_phase_grad(const void* gm, int64_t ldg, const void* h, int64_t ldh, const void* s_r, const void* s_i, const void* p_r, const void* p_i,
                         const void* kf, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride, int n_k, const void* damp,
                         const void* ddamp, const int64_t* ptr, int64_t n_graphs, void* g_theta, void* g_damp, void* g_pos, void* stream) {
  EwPhaseArgs a{};
  const int st = ew_geom("xeq_ewald_phase_grad", a.e, pos, kvec, kvec_gstride, n_k, damp, ptr, n_graphs, n, node_dim);
  if (st != XEQ_OK) return st;
  XEQ_CHECK_ARG(ldg >= node_dim && ldh >= node_dim, "xeq_ewald_phase_grad: row strides %lld, %lld", (long long)ldg, (long long)ldh);
  XEQ_CHECK_ARG(n == 0 || (gm && h && s_r && s_i && p_r && p_i && kf && g_pos && n_graphs >= 1), "xeq_ewald_phase_grad: null buffer or no graph");
  if (n == 0) return XEQ_OK;
  a.GM = (const float*)gm;
  a.H = (const float*)h;
  a.ldg = ldg;
  a.ldh = ldh;
  a.SR = (const float*)s_r;
  a.SI = (const float*)s_i;
  a.PR = (const float*)p_r;
  a.PI = (const float*)p_i;
  a.kf = (const float*)kf;
  a.ddamp = (const float*)ddamp;
  a.g_theta = (float*)g_theta;
  a.g_damp = (float*)g_damp;
  a.g_pos = (float*)g_pos;
  hipLaunchKernelGGL(k_ewald_phase, dim3((unsigned)(n / EW_CHUNK + n_graphs)), dim3(256), 0, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_ewald_phase_grad");
  return XEQ_OK;
}

int xeq_ewald_damping(const void* pos, int64_t n, double scale, double eps, void* damp, void* ddamp, void* stream) {
  XEQ_CHECK_ARG(n >= 0 && (n == 0 || (pos && damp)), "xeq_ewald_damping: null buffer");
  if (n == 0) return XEQ_OK;
  hipLaunchKernelGGL(k_ewald_damping, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)pos, n, (float)scale, (float)eps,
                     (float*)damp, (float*)ddamp);
  XEQ_CHECK_LAUNCH("xeq_ewald_damping");
  return XEQ_OK;
}

int xeq_ewald_layernorm_fwd(const void* x, int64_t n, int node_dim, const void* weight, const void* bias, double eps, void* y, void* stats, void* stream) {
  XEQ_CHECK_ARG(n >= 0 && node_dim >= 1 && node_dim <= 256, "xeq_ewald_layernorm_fwd: node_dim %d (<= 256)", node_dim);
  XEQ_CHECK_ARG(n == 0 || (x && weight && bias && y && stats), "xeq_ewald_layernorm_fwd: null buffer");
  if (n == 0) return XEQ_OK;
  hipLaunchKernelGGL(k_ewald_ln_fwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)x, n, node_dim, (const float*)weight,
                     (const float*)bias, (float)eps, (float*)y, (float*)stats);
  XEQ_CHECK_LAUNCH("xeq_ewald_layernorm_fwd");
  return XEQ_OK;
}

int xeq_ewald_layernorm_bwd(const void* g, const void* x, const void* stats, const void* weight, int64_t n, int node_dim, void* g_x, void* stream) {
  XEQ_CHECK_ARG(n >= 0 && node_dim >= 1 && node_dim <= 256, "xeq_ewald_layernorm_bwd: node_dim %d (<= 256)", node_dim);
  XEQ_CHECK_ARG(n == 0 || (g && x && stats && weight && g_x), "xeq_ewald_layernorm_bwd: null buffer");
  if (n == 0) return XEQ_OK;
  hipLaunchKernelGGL(k_ewald_ln_bwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)g, (const float*)x, (const float*)stats,
                     (const float*)weight, n, node_dim, (float*)g_x);
  XEQ_CHECK_LAUNCH("xeq_ewald_layernorm_bwd");
  return XEQ_OK;
}

int xeq_ewald_combine(const void* a, double sa, const void* b, double sb, const void* pre, int64_t count, void* out, void* stream) {
  XEQ_CHECK_ARG(count >= 0 && (count == 0 || (a && out)), "xeq_ewald_combine: null buffer");
  if (count == 0) return XEQ_OK;
  const int64_t blocks = (count + 255) / 256;
  hipLaunchKernelGGL(k_ewald_combine, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (const float*)a, (float)sa,
                     (const float*)b, (float)sb, (const float*)pre, count, (float*)out);
  XEQ_CHECK_LAUNCH("xeq_ewald_combine");
  return XEQ_OK;
}

}  // extern "C"
