// Property heads of XPaiNN behind the trunk (reference nn/output.py:28-76 ScalarOut, :131-179 AtomicChargesOut, :245-326 PolarOut with
// the Gate of nn/o3layer.py:47-75), f32 inference, two kernels.
//
// k_head_polar_nodes: PolarOut per node, one launch over tiles of 32 nodes (a workgroup of 4 waves per tile).
//   hs  = SiLU(W_s1 s_n + b_s1)                         [hidden_dim]      (a0, a2)_n = W_s2 hs + b_s2
//   h0  = W_0 x0_n / sqrt(mul0) + b_0                   [hid0]            x0: the 0e block of x_n
//   h2  = W_2 x2_n / sqrt(mul2)                         [hid2][5]         x2: the 2e block of x_n (the 1o block is not read)
//   gate: h[u, m] *= sigmoid(sqrt(sum_m h[u, m]^2 + eps^2) - eps)
//   t0  = <w_b0, g0> / sqrt(hid0) + b_b,  t2[m] = <w_b2, g2[:, m]> / sqrt(hid2)
//   t[n] = (a0 t0, a2 t2[0..5), 0, 0)
// The three hidden products are exact-f32 v_mfma_f32_32x32x2_f32 tiles with the conventions of xeq_linear.hip / xeq_electronic.hip:
// the weight fragment (a xeq_mlp_pack copy, output columns padded with zero rows to a multiple of 32, 1 / sqrt(mul) folded in) is the
// A operand, the row operand is staged in LDS; the 2e product has (node, m) as its 32 x 5 = 160 rows.  Wave w takes the jobs w, w + 4,
// ... of the tile's (hidden / 32 + hid0 / 32 + 5 hid2 / 32) output tiles.  The epilogue (SiLU is applied when the tile is written
// to LDS; gate, second linear layers, a0 / a2 weighting) runs eight threads per node over the LDS copies, columns sub, sub + 8, ...
// and a butterfly: one fixed order per node whatever the tile, the batch or the shard.  s and x are read with their row strides,
// rows past n are neither read nor written.
// Envelope (xeq_head_polar_supported): f32, SiLU; node_dim, mul0 multiples of 32, <= 256; mul2 a multiple of 8, <= 64; hidden_dim,
// hid0 multiples of 4, <= 128; hid2 a multiple of 4, <= 32; the tile's LDS (below) within 160 KB.
//
// k_head_graph_reduce: per-graph sums of up to 8 columns without atomics, one wave per graph: lane l adds the rows ptr[g] + l, + 64, ...
// and a fixed butterfly joins the lanes, so the order depends on the atom's index inside its graph alone and a graph's result is
// bit-identical alone, in a batch and in a shard.  mode 0 sum, 1 mean, 2 the polarizability tensor (nn/output.py:301-320), 3 charge
// conservation written back over the graph's rows.  An empty graph gives zeros and divides nothing.
#include "xeq_common.h"
#include "xeq_linear_s.h"

namespace xeq {

constexpr int HP_ROWS = 32;
static_assert(HP_ROWS == PW_ROWS, "stage_rows32 / pw_chain32 work on 32-row tiles");

struct PolarArgs {
  const float* S;        // [n, lds]
  const float* X;        // [n, ldx]; the 0e block at column 0, the 2e block at column off2
  int64_t lds, ldx, n;
  int F, mul0, mul2, off2;
  int H, H0, H2;         // hidden_dim, hid0, hid2 (true widths)
  int Hp, H0p, H2p;      // the same rounded up to multiples of 32 (the packed copies' widths)
  const float* Ws1p;     // xeq_mlp_pack([Hp, F], b_s1)
  const float* W0p;      // xeq_mlp_pack([H0p, mul0] / sqrt(mul0), b_0)
  const float* W2p;      // xeq_mlp_pack([H2p, mul2] / sqrt(mul2), NULL)
  const float* Ws2;      // [2, H]   scalar_out_mlp.2.weight
  const float* bs2;      // [2]
  const float* Wb;       // [H0 + H2] equi_out_mlp.2.weight (flat: the 0e block, then the 2e block)
  const float* bb;       // [1]
  float eps;
  float* T;              // [n, 8]
};

__host__ __device__ inline int hp_pad32(int v) { return (v + 31) & ~31; }
// floats of LDS per tile: s, x0, x2 rows and the three products
__host__ __device__ inline size_t hp_lds_floats(int F, int mul0, int mul2, int Hp, int H0p, int H2p) {
  return (size_t)HP_ROWS * ((F + 4) + (mul0 + 4) + 5 * (mul2 + 4) + (Hp + 4) + (H0p + 4) + 5 * (H2p + 4));
}

__device__ __forceinline__ float hp_gate(float sq, float eps) { return 1.f / (1.f + expf(-(sqrtf(sq + eps * eps) - eps))); }

__global__ void __launch_bounds__(256) k_head_polar_nodes(PolarArgs a) {
  extern __shared__ __attribute__((aligned(16))) float hp_lds[];
  const int SLD = a.F + 4, X0LD = a.mul0 + 4, X2LD = a.mul2 + 4, HLD = a.Hp + 4, H0LD = a.H0p + 4, H2LD = a.H2p + 4;
  float* Ss = hp_lds;                         // [32][F + 4]
  float* X0s = Ss + HP_ROWS * SLD;            // [32][mul0 + 4]
  float* X2s = X0s + HP_ROWS * X0LD;          // [5][32][mul2 + 4]   row (m, r): component m of node r
  float* Hs = X2s + 5 * HP_ROWS * X2LD;       // [32][Hp + 4]        SiLU(W_s1 s + b)
  float* H0s = Hs + HP_ROWS * HLD;            // [32][H0p + 4]
  float* H2s = H0s + HP_ROWS * H0LD;          // [5][32][H2p + 4]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, kh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * HP_ROWS;
  const int rows_here = (int)min((int64_t)HP_ROWS, a.n - row0);
  // stage s and the 0e block (16-byte loads; rows past n as zeros)
  stage_rows32(Ss, SLD, a.S, a.lds, row0, rows_here, a.F, tid);
  stage_rows32(X0s, X0LD, a.X, a.ldx, row0, rows_here, a.mul0, tid);
  // the 2e block [mul2][5] of a node, transposed to five rows of mul2 channels
  for_rows32(a.X + a.off2, a.ldx, row0, rows_here, 5 * a.mul2, tid, nullptr, [&](int r, int c4, const float4& v) {
    const float* pv = reinterpret_cast<const float*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = 4 * c4 + j, u = e / 5, m = e - 5 * u;
      X2s[(m * HP_ROWS + r) * X2LD + u] = pv[j];
    }
  });
  __syncthreads();
  const int nt_s = a.Hp >> 5, nt_0 = a.H0p >> 5, nt_2 = a.H2p >> 5;
  const int jobs = nt_s + nt_0 + 5 * nt_2;
  for (int job = wave; job < jobs; job += 4) {
    float* dst;
    f32x16 acc;
    int t;
    bool silu = false;
    if (job < nt_s) {
      t = job;
      acc = pw_tile_product32(a.Ws1p, t, a.F, &Ss[i * SLD + 4 * kh], lane, true);
      dst = &Hs[i * HLD];
      silu = true;
    } else if (job < nt_s + nt_0) {
      t = job - nt_s;
      acc = pw_tile_product32(a.W0p, t, a.mul0, &X0s[i * X0LD + 4 * kh], lane, true);
      dst = &H0s[i * H0LD];
    } else {
      const int j2 = job - nt_s - nt_0, m = j2 / nt_2;
      t = j2 - m * nt_2;
      acc = pw_tile_product32(a.W2p, t, a.mul2, &X2s[(m * HP_ROWS + i) * X2LD + 4 * kh], lane, false);
      dst = &H2s[(m * HP_ROWS + i) * H2LD];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = pw_quad(acc, g);
      if (silu) v = silu4(v);
      *reinterpret_cast<float4*>(dst + 32 * t + pw_quad_col(g, kh)) = v;
    }
  }
  __syncthreads();
  // epilogue: eight threads per node, columns sub, sub + 8, ...; then a butterfly over the eight
  const int r = tid >> 3, sub = tid & 7;
  float a0 = 0.f, a2 = 0.f, t0 = 0.f, t2[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = sub; c < a.H; c += 8) {
    const float h = Hs[r * HLD + c];
    a0 = fmaf(a.Ws2[c], h, a0);
    a2 = fmaf(a.Ws2[a.H + c], h, a2);
  }
  for (int c = sub; c < a.H0; c += 8) {
    const float h = H0s[r * H0LD + c];
    t0 = fmaf(a.Wb[c], h * hp_gate(h * h, a.eps), t0);
  }
  for (int c = sub; c < a.H2; c += 8) {
    float h[5], sq = 0.f;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      h[m] = H2s[(m * HP_ROWS + r) * H2LD + c];
      sq = fmaf(h[m], h[m], sq);
    }
    const float wg = a.Wb[a.H0 + c] * hp_gate(sq, a.eps);
#pragma unroll
    for (int m = 0; m < 5; ++m) t2[m] = fmaf(wg, h[m], t2[m]);
  }
  a0 = row_sum8(a0);
  a2 = row_sum8(a2);
  t0 = row_sum8(t0);
#pragma unroll
  for (int m = 0; m < 5; ++m) t2[m] = row_sum8(t2[m]);
  if (sub == 0 && r < rows_here) {
    a0 += a.bs2[0];
    a2 += a.bs2[1];
    const float i0 = 1.f / sqrtf((float)a.H0), i2 = 1.f / sqrtf((float)a.H2);
    t0 = fmaf(t0, i0, a.bb[0]);
    float* out = a.T + (row0 + r) * 8;
    *reinterpret_cast<float4*>(out) = make_float4(a0 * t0, a2 * (t2[0] * i2), a2 * (t2[1] * i2), a2 * (t2[2] * i2));
    *reinterpret_cast<float4*>(out + 4) = make_float4(a2 * (t2[3] * i2), a2 * (t2[4] * i2), 0.f, 0.f);
  }
}

struct ReduceArgs {
  float* src;            // [n, ld] (mode 3: rewritten in place)
  int64_t ld;
  const int64_t* ptr;    // [G + 1]
  int64_t G;
  int width, mode;
  const float* total;    // mode 3: [G] target charge or NULL (zero)
  float* out;            // modes 0, 1: [G, width]; mode 2: [G, 9]
  float* iso;            // mode 2: [G] or NULL
};

template <int W>
__device__ __forceinline__ void hr_graph(const ReduceArgs& a, int64_t g, int lane) {
  const int64_t b = a.ptr[g], e = a.ptr[g + 1];
  float acc[W];
#pragma unroll
  for (int c = 0; c < W; ++c) acc[c] = 0.f;
  for (int64_t p = b + lane; p < e; p += 64) {
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < a.width) acc[c] += a.src[p * a.ld + c];
  }
#pragma unroll
  for (int c = 0; c < W; ++c)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
  const int64_t cnt = e - b;
  if (a.mode == 0 || a.mode == 1) {
    const float scale = (a.mode == 1 && cnt > 0) ? (float)cnt : 1.f;
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (lane == c && c < a.width) a.out[g * a.width + c] = a.mode == 1 ? acc[c] / scale : acc[c];
  } else if (a.mode == 2) {
    if (lane == 0) {
      // z I + A from (z, dxy, dyz, dz2, dzx, dx2-y2), nn/output.py:301-320
      const float z = acc[0], dxy = acc[1 % W], dyz = acc[2 % W], dz2 = acc[3 % W], dzx = acc[4 % W], dx2 = acc[5 % W];
      const float dn = sqrtf(dxy * dxy + dyz * dyz + dz2 * dz2 + dzx * dzx + dx2 * dx2);
      const float is3 = 0.57735026918962576f;
      const float xx = z + (is3 * (dn - dz2) + dx2), yy = z + (is3 * (dn - dz2) - dx2), zz = z + is3 * (dn + 2.f * dz2);
      float* o = a.out + g * 9;
      o[0] = xx;
      o[1] = dxy;
      o[2] = dzx;
      o[3] = dxy;
      o[4] = yy;
      o[5] = dyz;
      o[6] = dzx;
      o[7] = dyz;
      o[8] = zz;
      if (a.iso) a.iso[g] = (xx + yy + zz) / 3.f;
    }
  } else if (cnt > 0) {   // mode 3
    const float delta = ((a.total ? a.total[g] : 0.f) - acc[0]) / (float)cnt;
    for (int64_t p = b + lane; p < e; p += 64) a.src[p * a.ld] += delta;
  }
}

__global__ void __launch_bounds__(256) k_head_graph_reduce(ReduceArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= a.G) return;
  if (a.width == 1) hr_graph<1>(a, g, lane);
  else hr_graph<8>(a, g, lane);
}

}  // namespace xeq

using namespace xeq;

static bool hp_shape_ok(int node_dim, int mul0, int mul2, int hidden_dim, int hid0, int hid2) {
  if (node_dim < 32 || node_dim > 256 || node_dim % 32 || mul0 < 32 || mul0 > 256 || mul0 % 32 || mul2 < 8 || mul2 > 64 || mul2 % 8) return false;
  if (hidden_dim < 4 || hidden_dim > 128 || hidden_dim % 4 || hid0 < 4 || hid0 > 128 || hid0 % 4 || hid2 < 4 || hid2 > 32 || hid2 % 4) return false;
  return sizeof(float) * hp_lds_floats(node_dim, mul0, mul2, hp_pad32(hidden_dim), hp_pad32(hid0), hp_pad32(hid2)) <= 160 * 1024;
}

extern "C" {

int xeq_head_polar_supported(int dtype, int node_dim, int mul0, int mul2, int hidden_dim, int hid0, int hid2) {
  return dtype == XEQ_F32 && hp_shape_ok(node_dim, mul0, mul2, hidden_dim, hid0, hid2) ? 1 : 0;
}

int xeq_head_polar_nodes(const void* s, int64_t lds, const void* x, int64_t ldx, int64_t n, int node_dim, int mul0, int mul2, int off2,
                         int hidden_dim, int hid0, int hid2, const void* ws1_packed, const void* w0_packed, const void* w2_packed,
                         const void* ws2, const void* bs2, const void* wb, const void* bb, double eps, void* t, void* stream) {
  XEQ_CHECK_ARG(n >= 0 && hp_shape_ok(node_dim, mul0, mul2, hidden_dim, hid0, hid2),
                "xeq_head_polar_nodes: widths (%d, %d, %d, %d, %d, %d) outside the envelope of xeq_head_polar_supported", node_dim, mul0, mul2,
                hidden_dim, hid0, hid2);
  XEQ_CHECK_ARG(lds >= node_dim && lds % 4 == 0, "xeq_head_polar_nodes: row stride of s %lld", (long long)lds);
  XEQ_CHECK_ARG(off2 >= mul0 && off2 % 4 == 0 && ldx >= (int64_t)off2 + 5 * mul2 && ldx % 4 == 0,
                "xeq_head_polar_nodes: row stride of x %lld, 2e block at %d", (long long)ldx, off2);
  XEQ_CHECK_ARG(n == 0 || (s && x && ws1_packed && w0_packed && w2_packed && ws2 && bs2 && wb && bb && t), "xeq_head_polar_nodes: null buffer");
  XEQ_CHECK_ARG(((uintptr_t)s % 16 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)t % 16 == 0), "xeq_head_polar_nodes: buffers must be 16-byte aligned");
  if (n == 0) return XEQ_OK;
  static const hipError_t lds_err = raise_dynamic_lds({reinterpret_cast<const void*>(&k_head_polar_nodes)}, 160 * 1024);
  XEQ_CHECK_ARG(lds_err == hipSuccess, "xeq_head_polar_nodes: cannot raise the dynamic LDS limit");
  PolarArgs a{(const float*)s, (const float*)x, lds, ldx, n, node_dim, mul0, mul2, off2, hidden_dim, hid0, hid2, hp_pad32(hidden_dim), hp_pad32(hid0),
              hp_pad32(hid2), (const float*)ws1_packed, (const float*)w0_packed, (const float*)w2_packed, (const float*)ws2, (const float*)bs2,
              (const float*)wb, (const float*)bb, (float)eps, (float*)t};
  const size_t shmem = sizeof(float) * hp_lds_floats(node_dim, mul0, mul2, a.Hp, a.H0p, a.H2p);
  hipLaunchKernelGGL(k_head_polar_nodes, dim3((unsigned)((n + HP_ROWS - 1) / HP_ROWS)), dim3(256), shmem, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_head_polar_nodes");
  return XEQ_OK;
}

int xeq_head_graph_reduce(int mode, void* src, int64_t ld, int width, const int64_t* ptr, int64_t n_graphs, const void* total, void* out,
                          void* iso, void* stream) {
  XEQ_CHECK_ARG(mode >= 0 && mode <= 3, "xeq_head_graph_reduce: mode %d (0 sum, 1 mean, 2 polar, 3 charge conservation)", mode);
  XEQ_CHECK_ARG(n_graphs >= 0 && width >= 1 && width <= 8 && ld >= width, "xeq_head_graph_reduce: width %d, row stride %lld", width, (long long)ld);
  XEQ_CHECK_ARG(mode != 2 || width == 6, "xeq_head_graph_reduce: the polar mode sums six columns (got %d)", width);
  XEQ_CHECK_ARG(mode != 3 || width == 1, "xeq_head_graph_reduce: charge conservation sums one column (got %d)", width);
  XEQ_CHECK_ARG(n_graphs == 0 || (src && ptr && (mode == 3 || out)), "xeq_head_graph_reduce: null buffer");
  if (n_graphs == 0) return XEQ_OK;
  ReduceArgs a{(float*)src, ld, ptr, n_graphs, width, mode, (const float*)total, (float*)out, (float*)iso};
  hipLaunchKernelGGL(k_head_graph_reduce, dim3((unsigned)((n_graphs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_head_graph_reduce");
  return XEQ_OK;
}

}  // extern "C"
