// Charge and spin embeddings (reference nn/electronic.py:13-90 with the bias-free ResidualLayer of nn/basic.py:11-31) in two launches
// per module, templated on the module's kind (0: charge, 1: spin).  Per graph g with total charge / spin t_g and node scalars s:
//   charge: a_g = relu([t_g, -t_g])      spin: a_g = [t_g]          key_in = a_g / max(a_g, 1), value_in = a_g
//   attn_n = softplus(<W_q s_n + b_q, W_k key_in(g(n))> / sqrt(F))                                  k_electronic_attn
//   c_n = attn_n W_v value_in(g(n)) / sum_{m in g(n)} attn_m
//   s_n <- s_n + (c_n + SiLU(W_2 SiLU(W_1 c_n))) / sqrt(2)                                            k_electronic_mix
// Design: the conventions of xeq_linear.hip.  A workgroup (4 waves) owns 32 consecutive nodes; exact-f32 v_mfma_f32_32x32x2_f32 tiles
// with the weight fragment (xeq_mlp_pack copy) as the A operand and the row operand staged in LDS.  A node's graph is found in `ptr`
// by binary search (graph_of, xeq_common.h).  The graph sums A_g of the mix pass are formed in every tile that touches the graph, by
// one wave, lane l adding the graph's entries ptr[g] + l, + 64, ... and a fixed butterfly: the order depends on the graph's own
// atoms alone, never on the tile, the batch or the shard, and no float atomics are used.  A row's sums run in one fixed order
// whatever the batch, so a molecule gets the same bits alone, inside a batch and inside a shard.
#include "xeq_common.h"
#include "xeq_linear_s.h"

namespace xeq {

constexpr int EL_ROWS = 32;
static_assert(EL_ROWS == PW_ROWS, "stage_rows32 / pw_chain32 work on 32-row tiles");

struct ElecArgs {
  const float* S;       // [n, lds] node scalars
  int64_t lds, n;
  int F;                // node_dim (multiple of 32, <= 256)
  const int64_t* ptr;   // [G + 1]
  int64_t G;
  const float* total;   // [G] total charge / spin of each graph
  const float* Wqp;     // xeq_mlp_pack(W_q, b_q, F, F, 0)
  const float* Wk;      // [F, KIN] (nn.Linear layout)
  const float* Wv;      // [F, KIN]
  const float* W1p;     // xeq_mlp_pack(residual.mlp[0].weight, NULL, F, F, 0)
  const float* W2p;     // xeq_mlp_pack(residual.mlp[2].weight, NULL, F, F, 0)
  float scale;          // 1 / sqrt(F)
  float inv_sqrt2;
  float* attn;          // [n]
  float* out;           // [n, F]
};

// (key_in, value_in) of a graph; KIND 0: charge [relu(t), relu(-t)], KIND 1: spin [t]
template <int KIND>
__device__ __forceinline__ void el_inputs(float t, float kin[2], float vin[2]) {
  if (KIND == 0) {
    vin[0] = fmaxf(t, 0.f);
    vin[1] = fmaxf(-t, 0.f);
  } else {
    vin[0] = t;
    vin[1] = 0.f;
  }
  kin[0] = vin[0] / fmaxf(vin[0], 1.f);
  kin[1] = vin[1] / fmaxf(vin[1], 1.f);
}

// attention pass: q = W_q s + b_q on the matrix cores, attn[n] = softplus(<q_n, k_g(n)> scale)
template <int KIND>
__global__ void __launch_bounds__(256) k_electronic_attn(ElecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float el_lds[];
  constexpr int KIN = KIND == 0 ? 2 : 1;
  const int XLD = a.F + 4;
  float* Xs = el_lds;                  // [32][F + 4] staged rows
  float* Qs = Xs + EL_ROWS * XLD;      // [32][F + 4] q
  __shared__ float kin_s[EL_ROWS][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, kh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * EL_ROWS;
  const int rows_here = (int)min((int64_t)EL_ROWS, a.n - row0);
  stage_rows32(Xs, XLD, a.S, a.lds, row0, rows_here, a.F, tid);
  if (tid < EL_ROWS) {
    float kin[2] = {0.f, 0.f}, vin[2];
    if (tid < rows_here) el_inputs<KIND>(a.total[graph_of(a.ptr, a.G, row0 + tid)], kin, vin);
    kin_s[tid][0] = kin[0];
    kin_s[tid][1] = kin[1];
  }
  __syncthreads();
  const float* xs = &Xs[i * XLD + 4 * kh];
  for (int t = wave; t < (a.F >> 5); t += 4) {
    const f32x16 acc = pw_tile_product32(a.Wqp, t, a.F, xs, lane, true);
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(&Qs[i * XLD + 32 * t + pw_quad_col(g, kh)]) = pw_quad(acc, g);
  }
  __syncthreads();
  // <q_n, k_g>: eight threads per row, columns sub, sub + 8, ... then a butterfly -- one fixed order per row
  const int r = tid >> 3, sub = tid & 7;
  const float k0 = kin_s[r][0], k1 = kin_s[r][1];
  float acc = 0.f;
  for (int c = sub; c < a.F; c += 8) {
    const float kc = KIN == 2 ? fmaf(a.Wk[2 * c + 1], k1, a.Wk[2 * c] * k0) : a.Wk[c] * k0;
    acc = fmaf(Qs[r * XLD + c], kc, acc);
  }
  acc = row_sum8(acc);
  if (sub == 0 && r < rows_here) {
    const float x = acc * a.scale;
    a.attn[row0 + r] = x > 20.f ? x : log1pf(expf(x));   // aten softplus (beta 1, threshold 20)
  }
}

// mix pass: A_g, c = attn v / A_g, the two bias-free Linear + SiLU layers, out = s + (c + mlp(c)) / sqrt(2)
template <int KIND>
__global__ void __launch_bounds__(256) k_electronic_mix(ElecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float el_lds[];
  constexpr int KIN = KIND == 0 ? 2 : 1;
  const int XLD = a.F + 4;
  float* Cs = el_lds;                  // [32][F + 4] c
  float* Hs = Cs + EL_ROWS * XLD;      // [32][F + 4] SiLU(W_1 c)
  __shared__ int64_t gid_s[EL_ROWS];
  __shared__ int lead_s[EL_ROWS];
  __shared__ float sum_s[EL_ROWS];
  __shared__ float vin_s[EL_ROWS][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, kh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * EL_ROWS;
  const int rows_here = (int)min((int64_t)EL_ROWS, a.n - row0);
  if (tid < EL_ROWS) {
    float kin[2], vin[2] = {0.f, 0.f};
    int64_t g = -1;
    if (tid < rows_here) {
      g = graph_of(a.ptr, a.G, row0 + tid);
      el_inputs<KIND>(a.total[g], kin, vin);
    }
    gid_s[tid] = g;
    vin_s[tid][0] = vin[0];
    vin_s[tid][1] = vin[1];
  }
  __syncthreads();
  if (tid < EL_ROWS) {   // the first row of this tile in the same graph: the graph's sum is kept there
    int l = tid;
    if (tid < rows_here)
      while (l > 0 && gid_s[l - 1] == gid_s[tid]) --l;
    lead_s[tid] = l;
  }
  __syncthreads();
  // A_g: one wave per graph of this tile, in the graph's own order (see the head comment)
  for (int r = wave; r < rows_here; r += 4) {
    if (lead_s[r] != r) continue;
    const int64_t g = gid_s[r], b = a.ptr[g], e = a.ptr[g + 1];
    float acc = 0.f;
    for (int64_t p = b + lane; p < e; p += 64) acc += a.attn[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) sum_s[r] = acc;
  }
  __syncthreads();
  // c[n, j] = (attn_n v_g[j]) / A_g
  for (int idx = tid; idx < EL_ROWS * a.F; idx += 256) {
    const int r = idx / a.F, col = idx - r * a.F;
    float c = 0.f;
    if (r < rows_here) {
      const float v = KIN == 2 ? fmaf(a.Wv[2 * col + 1], vin_s[r][1], a.Wv[2 * col] * vin_s[r][0]) : a.Wv[col] * vin_s[r][0];
      c = (a.attn[row0 + r] * v) / sum_s[lead_s[r]];
    }
    Cs[r * XLD + col] = c;
  }
  __syncthreads();
  const int nt = a.F >> 5;
  for (int t = wave; t < nt; t += 4) {
    const f32x16 acc = pw_tile_product32(a.W1p, t, a.F, &Cs[i * XLD + 4 * kh], lane, false);
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(&Hs[i * XLD + 32 * t + pw_quad_col(g, kh)]) = silu4(pw_quad(acc, g));
  }
  __syncthreads();
  for (int t = wave; t < nt; t += 4) {
    const f32x16 acc = pw_tile_product32(a.W2p, t, a.F, &Hs[i * XLD + 4 * kh], lane, false);
    if (i < rows_here) {
      const int64_t row = row0 + i;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * t + pw_quad_col(g, kh);
        const float4 sv = *reinterpret_cast<const float4*>(a.S + row * a.lds + col);
        const float4 cv = *reinterpret_cast<const float4*>(&Cs[i * XLD + col]);
        const float4 m = silu4(pw_quad(acc, g));
        float4 o;
        o.x = sv.x + a.inv_sqrt2 * (cv.x + m.x);
        o.y = sv.y + a.inv_sqrt2 * (cv.y + m.y);
        o.z = sv.z + a.inv_sqrt2 * (cv.z + m.z);
        o.w = sv.w + a.inv_sqrt2 * (cv.w + m.w);
        *reinterpret_cast<float4*>(a.out + row * a.F + col) = o;
      }
    }
  }
}

}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_electronic_supported(int dtype, int node_dim) {
  return dtype == XEQ_F32 && node_dim >= 32 && node_dim <= 256 && node_dim % 32 == 0 ? 1 : 0;
}

int xeq_electronic_fwd(int kind, const void* s, int64_t lds, int64_t n, int node_dim, const int64_t* ptr, int64_t n_graphs, const void* total,
                       const void* wq_packed, const void* w_k, const void* w_v, const void* w1_packed, const void* w2_packed, void* attn,
                       void* out, void* stream) {
  XEQ_CHECK_ARG(kind == 0 || kind == 1, "xeq_electronic_fwd: kind %d (0 charge, 1 spin)", kind);
  XEQ_CHECK_ARG(n >= 0 && xeq_electronic_supported(XEQ_F32, node_dim), "xeq_electronic_fwd: node_dim %d (multiples of 32, <= 256)", node_dim);
  XEQ_CHECK_ARG(lds >= node_dim && lds % 4 == 0, "xeq_electronic_fwd: row stride %lld", (long long)lds);
  XEQ_CHECK_ARG(n == 0 || (s && ptr && n_graphs >= 1 && total && wq_packed && w_k && w_v && w1_packed && w2_packed && attn && out),
                "xeq_electronic_fwd: null buffer or no graph");
  if (n == 0) return XEQ_OK;
  // dynamic LDS above the default 64 KB for node_dim 256 (2 x 32 x 260 floats + the static arrays)
  static const hipError_t lds_err =
      raise_dynamic_lds({reinterpret_cast<const void*>(&k_electronic_attn<0>), reinterpret_cast<const void*>(&k_electronic_attn<1>),
                         reinterpret_cast<const void*>(&k_electronic_mix<0>), reinterpret_cast<const void*>(&k_electronic_mix<1>)},
                        sizeof(float) * EL_ROWS * 2 * (256 + 4));
  XEQ_CHECK_ARG(lds_err == hipSuccess, "xeq_electronic_fwd: cannot raise the dynamic LDS limit");
  ElecArgs a{(const float*)s, lds, n, node_dim, ptr, n_graphs, (const float*)total, (const float*)wq_packed, (const float*)w_k,
             (const float*)w_v, (const float*)w1_packed, (const float*)w2_packed, (float)(1.0 / std::sqrt((double)node_dim)),
             (float)(1.0 / std::sqrt(2.0)), (float*)attn, (float*)out};
  const size_t shmem = sizeof(float) * (size_t)EL_ROWS * 2 * (node_dim + 4);
  const dim3 grid((unsigned)((n + EL_ROWS - 1) / EL_ROWS));
  if (kind == 0) hipLaunchKernelGGL(k_electronic_attn<0>, grid, dim3(256), shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_electronic_attn<1>, grid, dim3(256), shmem, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_electronic_attn");
  if (kind == 0) hipLaunchKernelGGL(k_electronic_mix<0>, grid, dim3(256), shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_electronic_mix<1>, grid, dim3(256), shmem, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_electronic_mix");
  return XEQ_OK;
}

}  // extern "C"
