// Edge geometry of an evaluation that is differentiated twice with respect to the positions (hessian.py): edge vector -> distance ->
// radial basis x envelope, spherical harmonics -> the per-edge record of the message kernels (xeq_edge_basis's layout)
//   [f rho_k (B) | 0 to a multiple of 4 | f | Y_1 (3) | Y_2 (5) | 0 0 0],
// with the values and conventions of the tensor chain of nn/training.py (radial_basis, envelope, spherical_harmonics: component
// normalisation, (y, z, x) order, norm clamped at 1e-12; envelope and all its derivatives zero at dist >= cutoff).
// As in xeq_train_node.hip there is ONE forward body and ONE reverse body, each evaluated on values or on dual numbers (value + tangent);
// the second order is the tangent of the reverse body (Hessians are symmetric), so no second-order formula is written by hand:
//   forward at tangent u                      = J(vec) u                         = d<u, dL/dvec>/dg_rec,
//   reverse at (vec + eps u, g_rec + eps w)   = tangent of J(vec)^T g_rec        = sum_k g_k Hess rec_k u + J^T w.
// The basis parameters (freq / mean, std) are inputs only: no parameter gradient.  f32 and f64, a thread per edge: the pass these kernels
// serve is bound by the message kernels and the library GEMMs around them; what they remove is the several dozen elementwise launches of
// the tensor chain per order.
#include "xeq_common.h"

namespace xeq {
namespace te {

template <typename T>
struct Dual {
  T v, d;
  __device__ __forceinline__ Dual() {}
  __device__ __forceinline__ Dual(T v_) : v(v_), d(T(0)) {}
  __device__ __forceinline__ Dual(T v_, T d_) : v(v_), d(d_) {}
};
#define XEQ_TE_OP __device__ __forceinline__
template <typename T> XEQ_TE_OP Dual<T> operator+(Dual<T> a, Dual<T> b) { return {a.v + b.v, a.d + b.d}; }
template <typename T> XEQ_TE_OP Dual<T> operator-(Dual<T> a, Dual<T> b) { return {a.v - b.v, a.d - b.d}; }
template <typename T> XEQ_TE_OP Dual<T> operator-(Dual<T> a) { return {-a.v, -a.d}; }
template <typename T> XEQ_TE_OP Dual<T> operator*(Dual<T> a, Dual<T> b) { return {a.v * b.v, a.v * b.d + a.d * b.v}; }
template <typename T> XEQ_TE_OP Dual<T> operator/(Dual<T> a, Dual<T> b) {
  const T q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
template <typename T> XEQ_TE_OP Dual<T> operator+(Dual<T> a, T b) { return {a.v + b, a.d}; }
template <typename T> XEQ_TE_OP Dual<T> operator-(Dual<T> a, T b) { return {a.v - b, a.d}; }
template <typename T> XEQ_TE_OP Dual<T> operator*(Dual<T> a, T b) { return {a.v * b, a.d * b}; }
template <typename T> XEQ_TE_OP Dual<T> operator*(T b, Dual<T> a) { return {a.v * b, a.d * b}; }
template <typename T> XEQ_TE_OP Dual<T> operator/(Dual<T> a, T b) { return {a.v / b, a.d / b}; }
template <typename T> XEQ_TE_OP Dual<T>& operator+=(Dual<T>& a, Dual<T> b) {
  a.v += b.v;
  a.d += b.d;
  return a;
}

XEQ_TE_OP float val(float x) { return x; }
XEQ_TE_OP double val(double x) { return x; }
template <typename T> XEQ_TE_OP T val(Dual<T> x) { return x.v; }

XEQ_TE_OP float sqrt_s(float x) { return sqrtf(x); }
XEQ_TE_OP double sqrt_s(double x) { return sqrt(x); }
template <typename T> XEQ_TE_OP Dual<T> sqrt_s(Dual<T> x) {
  const T r = sqrt_s(x.v);
  return {r, x.d / (T(2) * r)};
}
XEQ_TE_OP float sin_s(float x) { return sinf(x); }
XEQ_TE_OP double sin_s(double x) { return sin(x); }
XEQ_TE_OP float cos_s(float x) { return cosf(x); }
XEQ_TE_OP double cos_s(double x) { return cos(x); }
template <typename T> XEQ_TE_OP Dual<T> sin_s(Dual<T> x) { return {sin_s(x.v), cos_s(x.v) * x.d}; }
template <typename T> XEQ_TE_OP Dual<T> cos_s(Dual<T> x) { return {cos_s(x.v), -sin_s(x.v) * x.d}; }
XEQ_TE_OP float exp_s(float x) { return expf(x); }
XEQ_TE_OP double exp_s(double x) { return exp(x); }
template <typename T> XEQ_TE_OP Dual<T> exp_s(Dual<T> x) {
  const T e = exp_s(x.v);
  return {e, e * x.d};
}
XEQ_TE_OP float abs_s(float x) { return fabsf(x); }
XEQ_TE_OP double abs_s(double x) { return fabs(x); }
// clamp_min of the norm: below the floor the value is the constant
XEQ_TE_OP float floor_s(float x, float lo) { return x < lo ? lo : x; }
XEQ_TE_OP double floor_s(double x, double lo) { return x < lo ? lo : x; }
template <typename T> XEQ_TE_OP Dual<T> floor_s(Dual<T> x, T lo) { return x.v < lo ? Dual<T>(lo) : x; }

// value (+ tangent, which may be absent = zero) in, value or tangent out
template <typename T, bool DUAL>
struct Acc;
template <typename T>
struct Acc<T, false> {
  using S = T;
  static XEQ_TE_OP S ld(const T* __restrict__ p, const T* __restrict__, int64_t i) { return p[i]; }
  static XEQ_TE_OP void st(T* __restrict__ o, int64_t i, S v) { o[i] = v; }
};
template <typename T>
struct Acc<T, true> {
  using S = Dual<T>;
  static XEQ_TE_OP S ld(const T* __restrict__ p, const T* __restrict__ t, int64_t i) { return S(p[i], t ? t[i] : T(0)); }
  static XEQ_TE_OP void st(T* __restrict__ o, int64_t i, S v) { o[i] = v.d; }
};

template <typename T>
struct EdgeArgs {
  int64_t E;
  const T *vec, *vec_t, *g, *g_t, *p0, *p1;
  T* out;
  int rbf_kind, cutoff_kind, B, W;
  T cutoff, coeff;   // coeff: sqrt(2 / cutoff) of the Bessel basis
};

constexpr double kPi = 3.14159265358979323846;
constexpr double kBasisEps = 1e-5;    // eps of SphericalBesselj0 / GaussianSmearing (nn/rbf.py)
constexpr double kNormFloor = 1e-12;  // clamp of the harmonics' norm

// rho_k(d) and, with DERIV, d rho_k / dd
template <typename T, typename S, bool DERIV>
XEQ_TE_OP void basis_fn(const EdgeArgs<T>& a, int k, S d, S& rho, S& drho) {
  if (a.rbf_kind == XEQ_RBF_BESSEL) {
    const T w = a.p0[k];
    const S den = d + T(kBasisEps);
    const S sn = sin_s(d * w);
    rho = sn * a.coeff / den;
    if (DERIV) drho = (cos_s(d * w) * (w * a.coeff) - rho) / den;
  } else {
    const T sd = abs_s(a.p1[k]) + T(kBasisEps);
    const S t = (d - a.p0[k]) / sd;
    rho = exp_s(t * t * T(-0.5)) / (sd * T(2.5066282746310002));   // sqrt(2 pi)
    if (DERIV) drho = -(rho * t) / sd;
  }
}

// f(d) and f'(d) inside the cutoff
template <typename T, typename S, bool DERIV>
XEQ_TE_OP void envelope_fn(const EdgeArgs<T>& a, S d, S& f, S& df) {
  if (a.cutoff_kind == XEQ_CUTOFF_COSINE) {
    const S x = d * T(kPi) / a.cutoff;
    f = (cos_s(x) + T(1)) * T(0.5);
    if (DERIV) df = sin_s(x) * (T(-0.5) * T(kPi) / a.cutoff);
  } else {
    const S r = d / a.cutoff;
    const S r2 = r * r, r3 = r2 * r;
    f = S(T(1)) - r3 * T(10) + r3 * r * T(15) - r3 * r2 * T(6);
    if (DERIV) df = (r3 * T(60) - r2 * T(30) - r2 * r2 * T(30)) / a.cutoff;
  }
}

template <typename T, bool DUAL>
__global__ void __launch_bounds__(256) k_edge_fwd(EdgeArgs<T> a) {
  using A = Acc<T, DUAL>;
  using S = typename A::S;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const S v0 = A::ld(a.vec, a.vec_t, 3 * e), v1 = A::ld(a.vec, a.vec_t, 3 * e + 1), v2 = A::ld(a.vec, a.vec_t, 3 * e + 2);
  const S d = sqrt_s(v0 * v0 + v1 * v1 + v2 * v2);
  T* row = a.out + e * a.W;
  const int bp = (a.B + 3) & ~3;
  const bool inside = val(d) < a.cutoff;
  S f = S(T(0)), unused;
  if (inside) envelope_fn<T, S, false>(a, d, f, unused);
  for (int k = 0; k < a.B; ++k) {
    S rho = S(T(0));
    if (inside) {
      basis_fn<T, S, false>(a, k, d, rho, unused);
      rho = rho * f;
    }
    A::st(row, k, rho);
  }
  for (int k = a.B; k < bp; ++k) row[k] = T(0);
  A::st(row, bp, f);
  const S n = floor_s(d, T(kNormFloor));
  const S x = v1 / n, y = v2 / n, z = v0 / n;   // e3nn's (x, y, z) are the edge vector's (y, z, x)
  const T s3 = T(1.7320508075688772), c15 = T(3.8729833462074170), c5 = T(2.2360679774997898);
  A::st(row, bp + 1, x * s3);
  A::st(row, bp + 2, y * s3);
  A::st(row, bp + 3, z * s3);
  A::st(row, bp + 4, x * z * c15);
  A::st(row, bp + 5, x * y * c15);
  A::st(row, bp + 6, (y * y - (x * x + z * z) * T(0.5)) * c5);
  A::st(row, bp + 7, y * z * c15);
  A::st(row, bp + 8, (z * z - x * x) * (T(0.5) * c15));
  row[bp + 9] = T(0);
  row[bp + 10] = T(0);
  row[bp + 11] = T(0);
}

template <typename T, bool DUAL>
__global__ void __launch_bounds__(256) k_edge_bwd(EdgeArgs<T> a) {
  using A = Acc<T, DUAL>;
  using S = typename A::S;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const S v0 = A::ld(a.vec, a.vec_t, 3 * e), v1 = A::ld(a.vec, a.vec_t, 3 * e + 1), v2 = A::ld(a.vec, a.vec_t, 3 * e + 2);
  const S d = sqrt_s(v0 * v0 + v1 * v1 + v2 * v2);
  const int64_t r0 = e * a.W;
  const int bp = (a.B + 3) & ~3;
  // dL/dd through the record head (f rho_k | f); beyond the cutoff the radial part and every derivative of it are zero
  S gd = S(T(0));
  if (val(d) < a.cutoff) {
    S f, df;
    envelope_fn<T, S, true>(a, d, f, df);
    gd = A::ld(a.g, a.g_t, r0 + bp) * df;
    for (int k = 0; k < a.B; ++k) {
      S rho, drho;
      basis_fn<T, S, true>(a, k, d, rho, drho);
      gd += A::ld(a.g, a.g_t, r0 + k) * (drho * f + rho * df);
    }
  }
  // dL/du of the unit vector u = (z, x, y) through the harmonics
  const S n = floor_s(d, T(kNormFloor));
  const S x = v1 / n, y = v2 / n, z = v0 / n;
  const T s3 = T(1.7320508075688772), c15 = T(3.8729833462074170), c5 = T(2.2360679774997898);
  S g1[3], g2[5];
  for (int m = 0; m < 3; ++m) g1[m] = A::ld(a.g, a.g_t, r0 + bp + 1 + m);
  for (int m = 0; m < 5; ++m) g2[m] = A::ld(a.g, a.g_t, r0 + bp + 4 + m);
  const S gx = g1[0] * s3 + (z * g2[0] + y * g2[1] - x * g2[4]) * c15 - x * g2[2] * c5;
  const S gy = g1[1] * s3 + (x * g2[1] + z * g2[3]) * c15 + y * g2[2] * (T(2) * c5);
  const S gz = g1[2] * s3 + (x * g2[0] + y * g2[3] + z * g2[4]) * c15 - z * g2[2] * c5;
  // u = vec / n: with the norm above its floor n = d depends on vec, below it n is the constant
  S o0 = gz / n, o1 = gx / n, o2 = gy / n;
  if (val(d) >= T(kNormFloor)) {
    const S radial = (gx * x + gy * y + gz * z) / n;
    o0 = o0 - z * radial;
    o1 = o1 - x * radial;
    o2 = o2 - y * radial;
  }
  // d = |vec|: dd/dvec = vec / d
  const S gdd = gd / d;
  A::st(a.out, 3 * e, o0 + v0 * gdd);
  A::st(a.out, 3 * e + 1, o1 + v1 * gdd);
  A::st(a.out, 3 * e + 2, o2 + v2 * gdd);
}

}  // namespace te
}  // namespace xeq

using namespace xeq;
using namespace xeq::te;

extern "C" {

int xeq_train_edge_supported(int dtype, int rbf_kind, int cutoff_kind, int num_basis) {
  return ((dtype == XEQ_F32 || dtype == XEQ_F64) && (rbf_kind == XEQ_RBF_BESSEL || rbf_kind == XEQ_RBF_GAUSSIAN) &&
          (cutoff_kind == XEQ_CUTOFF_COSINE || cutoff_kind == XEQ_CUTOFF_POLYNOMIAL) && num_basis >= 1 && num_basis <= 32)
             ? 1
             : 0;
}

int xeq_train_edge(int dtype, int reverse, int64_t n_edges, const void* vec, const void* vec_tan, const void* g_rec, const void* g_rec_tan,
                   int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1, void* out, void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_train_edge: unsupported dtype %d", dtype);
  XEQ_CHECK_ARG(n_edges >= 0 && n_edges < (1ll << 31) && cutoff > 0, "xeq_train_edge: bad sizes");
  XEQ_CHECK_ARG(num_basis >= 1 && num_basis <= 32, "xeq_train_edge: num_basis %d is outside 1..32", num_basis);
  XEQ_CHECK_ARG(rbf_kind == XEQ_RBF_BESSEL || rbf_kind == XEQ_RBF_GAUSSIAN,
                "xeq_train_edge: radial basis %d has no kernel form (Bessel and Gaussian only: xeq_train_edge_supported)", rbf_kind);
  XEQ_CHECK_ARG(cutoff_kind == XEQ_CUTOFF_COSINE || cutoff_kind == XEQ_CUTOFF_POLYNOMIAL, "xeq_train_edge: cutoff function %d is not implemented",
                cutoff_kind);
  XEQ_CHECK_ARG(vec && out && p0, "xeq_train_edge: vec, out and p0 must be given");
  XEQ_CHECK_ARG(rbf_kind == XEQ_RBF_BESSEL || p1 != nullptr, "xeq_train_edge: the Gaussian basis needs its second parameter array (std)");
  XEQ_CHECK_ARG(!reverse || g_rec, "xeq_train_edge: the reverse form needs g_rec");
  XEQ_CHECK_ARG(reverse || (g_rec == nullptr && g_rec_tan == nullptr), "xeq_train_edge: the forward form takes no g_rec");
  if (n_edges == 0) return XEQ_OK;
  const bool dual = vec_tan != nullptr || (reverse && g_rec_tan != nullptr);
  const dim3 grid((unsigned)((n_edges + 255) / 256));
  XEQ_DISPATCH_FLOAT(dtype, {
    EdgeArgs<T> a{n_edges,   (const T*)vec, (const T*)vec_tan, (const T*)g_rec, (const T*)g_rec_tan, (const T*)p0, (const T*)p1, (T*)out,
                  rbf_kind,  cutoff_kind,   num_basis,         ((num_basis + 3) & ~3) + 12,          (T)cutoff,    (T)sqrt(2.0 / cutoff)};
    if (!reverse) {
      if (dual) hipLaunchKernelGGL((k_edge_fwd<T, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
      else hipLaunchKernelGGL((k_edge_fwd<T, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
      if (dual) hipLaunchKernelGGL((k_edge_bwd<T, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
      else hipLaunchKernelGGL((k_edge_bwd<T, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
  });
  XEQ_CHECK_LAUNCH("xeq_train_edge");
  return XEQ_OK;
}

}  // extern "C"
