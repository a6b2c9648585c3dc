// The packed weight format of the exact-f32 matrix-core kernels on the node side, its writer's index arithmetic and its readers.
//
//   packed[tile of 32 outputs][k-group of 8 (+ one bias group)][lane][4] = W[32 tile + (lane & 31)][8 group + 4 (lane >> 5) + j]
//
// One coalesced 16-byte load per lane feeds four steps of v_mfma_f32_32x32x2_f32 with the WEIGHT fragment as the A operand (the k
// order inside a group of 8 is a permutation, applied to both operands); the bias is one more k-group, multiplied by a row of ones.
// The few-row forms read the SAME copy for v_mfma_f32_16x16x4_f32: lane (i, kq) of a 16-column half tile takes
// k = 8 q + 4 (kq & 1) + 2 s + (kq >> 1), s = 0, 1 -- the order in which the 32-row form's four instructions of a k-group visit the
// eight k -- so both forms run the same fused-multiply-add chain per output element and give the same bits (xeq_linear_s.h).
// Header only: the vector types, the small elementwise forms and the LDS helpers the readers share sit here too.
#pragma once
#include "xeq_common.h"

namespace xeq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains this wave's global stores and prefetches (vmcnt(0))
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// exp: the library's expf (<= 1 ulp, what the reference's SiLU evaluates).  (The hardware exp2 path, ~2 ulp + the rounding of x log2 e:
// the accuracy / time comparison of DESIGN section 2.)
__device__ __forceinline__ float silu_f(float x) {
  return x / (1.f + expf(-x));
}
__device__ __forceinline__ float silu_grad_f(float x) {  // aten silu_backward: sig (1 + x (1 - sig))
  const float sig = 1.f / (1.f + expf(-x));
  return sig * (1.f + x * (1.f - sig));
}
__device__ __forceinline__ float4 silu4(const float4& v) { return make_float4(silu_f(v.x), silu_f(v.y), silu_f(v.z), silu_f(v.w)); }

// ---- the writer's side: which weights float4 `idx` of the packed buffer holds (G = k_in / 8 k-groups, then the bias group) -------------
struct PwSlot {
  int n, k0;      // output row and first of the four k of this float4
  bool bias;      // the bias group: .x of the kh = 0 lanes holds bias[n], the rest zeros
  bool bias_lane;
};
__host__ __device__ inline int64_t pw_float4s(int n_out, int G) { return (int64_t)(n_out / 32) * (G + 1) * 64; }
__host__ __device__ inline PwSlot pw_slot(int64_t idx, int G) {
  const int lane = (int)(idx & 63);
  const int64_t tq = idx >> 6;
  const int q = (int)(tq % (G + 1)), t = (int)(tq / (G + 1));
  return PwSlot{32 * t + (lane & 31), 8 * q + 4 * (lane >> 5), q == G, (lane >> 5) == 0};
}

// ---- the readers' side ------------------------------------------------------------------------------------------------------------------
// first fragment of output tile t (wave-uniform; a 32-row reader adds its lane)
__device__ __forceinline__ const float4* pw_tile32(const float* Wp, int64_t t, int G) {
  return reinterpret_cast<const float4*>(Wp) + t * (G + 1) * 64;
}
// this lane's slot in the packed 32-column tile that holds the 16-column half tile t16 (lane = i + 16 kq, kh = kq & 1)
__device__ __forceinline__ const float4* pw_half16(const float4* tile32, int t16, int i, int kh) { return tile32 + 16 * (t16 & 1) + i + 32 * kh; }
__device__ __forceinline__ const float4* pw_tile16(const float* Wp, int t16, int G, int i, int kh) {
  return pw_half16(pw_tile32(Wp, t16 >> 1, G), t16, i, kh);
}
// the two k a 16x16x4 lane takes of a fragment (sel = kq >> 1), first and second instruction of the k-group; the row operand likewise
__device__ __forceinline__ float pw_pick0(bool sel, const float4& v) { return sel ? v.y : v.x; }
__device__ __forceinline__ float pw_pick1(bool sel, const float4& v) { return sel ? v.w : v.z; }
// the bias element of a lane (the lanes with kh = 0 hold the bias, the others zero): frag = the lane's first fragment of its tile, or
// the tile's with the lane's offset in `lane`; G groups on from there
__device__ __forceinline__ float pw_bias(const float4* frag, int64_t G, int lane = 0) {
  return reinterpret_cast<const float*>(frag + G * 64 + lane)[0];
}

// W x over the k-groups [q0, q1) for one output tile of 32 staged rows: one k-chain.  frag: pw_tile32 + lane; xs: this lane's staged
// row + 4 kh.  Weight fragments four k-groups ahead of their MFMAs (an L2 round trip is ~500 cycles, a group's four MFMAs 256), the
// prefetch clamped at the range's last group.  (The clamps are written out: behind a lambda `q < q1 ? q : q1 - 1` the compiler
// formed each fragment's address in front of its load instead of an iteration ahead, 3-9 % on the electronic kernels.)
__device__ __forceinline__ f32x16 pw_chain32(const float4* __restrict__ frag, const float* xs, int q0, int q1) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float4 w0 = frag[q0 * 64], w1 = frag[(q0 + 1 < q1 ? q0 + 1 : q1 - 1) * 64], w2 = frag[(q0 + 2 < q1 ? q0 + 2 : q1 - 1) * 64],
         w3 = frag[(q0 + 3 < q1 ? q0 + 3 : q1 - 1) * 64];
  for (int q = q0; q < q1; ++q) {
    const float4 wn = frag[(q + 4 < q1 ? q + 4 : q1 - 1) * 64];
    const float4 xv = *reinterpret_cast<const float4*>(xs + 8 * q);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.x, xv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.y, xv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.z, xv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.w, xv.w, acc, 0, 0, 0);
    w0 = w1;
    w1 = w2;
    w2 = w3;
    w3 = wn;
  }
  return acc;
}
// the bias rides in the product: one more k step whose weight fragment is the bias (k slot 0) against a row of ones (one_k0: 1 in the
// kh = 0 lanes, else 0)
__device__ __forceinline__ f32x16 pw_bias_step32(f32x16 acc, const float4* __restrict__ frag, int G, float one_k0) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(pw_bias(frag, G), one_k0, acc, 0, 0, 0);
}
// the whole product of a tile: every k-group, then the bias group
__device__ __forceinline__ f32x16 pw_tile_product32(const float* __restrict__ Wp, int t, int K, const float* xs, int lane, bool bias) {
  const int G = K >> 3;
  const float4* frag = pw_tile32(Wp, t, G) + lane;
  f32x16 acc = pw_chain32(frag, xs, 0, G);
  if (bias) acc = pw_bias_step32(acc, frag, G, (lane >> 5) == 0 ? 1.f : 0.f);
  return acc;
}

// accumulator layout (weights as the A operand): lane (row i, kh), register 4 g + e <-> column 8 g + 4 kh + e of the tile: four
// consecutive columns of one row per register quad, i.e. 16-byte stores / LDS writes straight from registers
__device__ __forceinline__ float4 pw_quad(const f32x16& acc, int g) { return make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]); }
__device__ __forceinline__ int pw_quad_col(int g, int kh) { return 8 * g + 4 * kh; }

// A row tile of these kernels: 32 rows, staged by a workgroup of 256 threads (four waves; the callers' __launch_bounds__(256) and
// their static_asserts on their own row constants hold them to it).
constexpr int PW_ROWS = 32, PW_THREADS = 256;
// PW_ROWS rows of K floats (K a multiple of 4) from src[(row0 + r) * stride ...] -- or from the rows row_index names -- handed to
// put(r, c4, float4) by the whole workgroup with 16-byte loads; rows past rows_here come as zeros and are not read
template <typename Put>
__device__ __forceinline__ void for_rows32(const float* __restrict__ src, int64_t stride, int64_t row0, int rows_here, int K, int tid,
                                           const int32_t* __restrict__ row_index, const Put& put) {
  const int k4 = K >> 2;   // float4 per row
  for (int idx = tid; idx < PW_ROWS * k4; idx += PW_THREADS) {
    const int r = idx / k4, c4 = idx - r * k4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows_here) {
      int64_t s = row0 + r;
      if (row_index) s = row_index[s];
      v = *reinterpret_cast<const float4*>(src + s * stride + 4 * c4);
    }
    put(r, c4, v);
  }
}
// the same rows staged in LDS as dst[r * ld + c]
__device__ __forceinline__ void stage_rows32(float* dst, int ld, const float* __restrict__ src, int64_t stride, int64_t row0, int rows_here,
                                             int K, int tid, const int32_t* __restrict__ row_index = nullptr) {
  for_rows32(src, stride, row0, rows_here, K, tid, row_index,
             [&](int r, int c4, const float4& v) { *reinterpret_cast<float4*>(&dst[r * ld + 4 * c4]) = v; });
}

// sum over the eight threads of a row (tid = 8 row + sub): a butterfly, one fixed order per row
__device__ __forceinline__ float row_sum8(float v) {
  v += __shfl_xor(v, 4, 8);
  v += __shfl_xor(v, 2, 8);
  v += __shfl_xor(v, 1, 8);
  return v;
}

}  // namespace xeq
