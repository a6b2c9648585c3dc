// Batched harmonic analysis behind the Hessian front (xequinet_amd/vibrations.py; the stage the reference hands to
// pyscf at run/geometry.py:210-237).  Five kernels, all f64 whatever the Hessian's dtype, one workgroup per graph, no atomics: a graph's
// result depends on no other graph of the launch and has the same bits alone and anywhere in a batch.
//
// k_vib_project (global memory, no size cap), per graph of n atoms, m = 3 n:
//   total mass, centre of mass and inertia tensor summed in atom order by one lane; principal moments (ascending) and axes by a 3 x 3
//   cyclic Jacobi in that lane; rotor class ATOM (n == 1), LINEAR (smallest moment <= 1e-6 x the largest) or NONLINEAR.
//   Q [n_tr, m]: the mass-weighted translations, then the rotations about the principal axes with a non-vanishing moment (a linear
//   molecule: the two larger ones), orthonormalised by modified Gram-Schmidt in that order; n_tr = 3 (atom, or `periodic`), 5, 6.
//   S = m^-1/2 (H + H^T)/2 m^-1/2;  W = S Q, C = Q^T W, Y = W - Q C / 2;  P S P = S - Q Y^T - Y Q^T (P = I - Q Q^T): O(n_tr m^2).
//   sigma = 2 |P S P|_F (1 when that is 0);  M = P S P + sigma Q Q^T.  Every eigenvalue of P S P is below sigma in magnitude, so the n_tr
//   rigid-body directions are the top of M's spectrum and the vibrations its lowest m - n_tr eigenpairs.
//   Every sum over a vector runs thread t over the entries t, t + 256, ... and a fixed tree over the 256 threads; M is computed on the
//   upper triangle and mirrored, so it is symmetric to the bit.
//
// k_vib_eigh: ragged batch of symmetric matrices of dimension m <= XEQ_VIB_MAX_DIM, one workgroup of 256 threads per matrix, A and V^T
//   resident in LDS with an odd leading dimension ld = m | 1.  8-byte LDS accesses are served 32 lanes at a time from 64 4-byte banks:
//   consecutive lanes on consecutive entries of a row are conflict-free, and a column walk with stride ld doubles is conflict-free
//   exactly when ld is odd.  V is kept transposed (vector k contiguous, the output's layout), so its update is a row update.
//   Two-sided cyclic Jacobi, round-robin ordering: mm = m rounded up to even, mm - 1 steps per sweep of mm / 2 disjoint pairs (pair 0 of
//   step s is (mm - 1, s), pair k is ((s + k) mod (mm - 1), (s - k) mod (mm - 1)); the pair with index m of an odd m idles).  Per step:
//   rotations from (a_pp, a_qq, a_pq) into LDS tables | barrier | columns of A | barrier | rows of A and of V^T, where a_pq = a_qp = 0
//   and a_pp -= t a_pq, a_qq += t a_pq are stored as such | barrier.  A pair with |a_pq| <= 2^-53 sqrt(|a_pp a_qq|) is skipped; the
//   smaller-angle root (|t| <= 1) is always taken, so diagonal entries never swap places.
//   Stop rule: off(A) = sqrt(sum_{i != j} a_ij^2), summed from the off-diagonal entries themselves (never as |A|^2 - sum a_ii^2, which
//   cannot see below sqrt(u) |A|), before every sweep; stop at off <= m 2^-53 |A|_F, or after XEQ_VIB_MAX_SWEEPS sweeps with status 1.
//   Output: eigenvalues ascending (equal ones by index), vector k contiguous, its largest-magnitude component (lowest index on a tie)
//   positive.
//
// k_vib_eigh_large: the same contract for XEQ_VIB_MAX_DIM < m <= XEQ_VIB_LARGE_MAX_DIM (any m >= 1 is accepted), one workgroup per matrix
//   working in the matrix's block of the output in global memory: Householder tridiagonalisation with accumulated Q, then implicit-shift
//   QL with the rotations applied to Q^T (described at the kernel).  It reads `mat` and leaves it as it was.
//
// k_vib_finish: from the lowest m - n_tr eigenpairs: eigenvalue, norm_mode = m_i^-1/2 v, reduced mass 1 / sum norm_mode^2, wavenumber
//   sign(lambda) sqrt(|lambda|) x factor (an imaginary mode negative: run/geometry.py:142), vibrational temperature, force constant,
//   and the count of negative eigenvalues.  One wave per mode, lanes over the entries and a butterfly.
// k_vib_thermo_sums: per graph the four RRHO sums over the modes with lambda > 0 at one temperature, one wave per graph.
#include <math.h>

#include "xeq_common.h"

namespace xeq {

constexpr int VIB_THREADS = 256;
constexpr int VIB_BATCH = 4;     // entries of a Jacobi phase a thread has in flight (k_vib_eigh)

// Sum of one value per thread over the workgroup in a fixed tree; every thread gets the total.  red: [VIB_THREADS] doubles of LDS.
__device__ __forceinline__ double vib_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // the previous total may still be being read
  red[t] = v;
  __syncthreads();
  for (int o = VIB_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// (c, s, t) of the Jacobi rotation that annihilates a_pq, smaller angle: theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
// sqrt(theta^2 + 1)); an overflowing theta^2 gives t = 0
__device__ __forceinline__ void vib_rotation(double app, double aqq, double apq, double& c, double& s, double& t) {
  const double th = (aqq - app) / (2.0 * apq);
  t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
}

// Principal moments (ascending) and axes (rows of ax) of a symmetric 3 x 3 tensor by cyclic Jacobi, one lane.
__device__ void vib_jacobi3(double I[3][3], double* mom, double* ax) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = I[0][1] * I[0][1] + I[0][2] * I[0][2] + I[1][2] * I[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = I[p][q];
        if (!(fabs(apq) > 0x1p-53 * sqrt(fabs(I[p][p] * I[q][q])))) {
          I[p][q] = I[q][p] = 0.0;
          continue;
        }
        double c, s, t;
        vib_rotation(I[p][p], I[q][q], apq, c, s, t);
        const double npp = I[p][p] - t * apq, nqq = I[q][q] + t * apq;
        for (int i = 0; i < 3; ++i) {
          const double x = I[i][p], y = I[i][q];
          I[i][p] = c * x - s * y;
          I[i][q] = s * x + c * y;
        }
        for (int j = 0; j < 3; ++j) {
          const double x = I[p][j], y = I[q][j];
          I[p][j] = c * x - s * y;
          I[q][j] = s * x + c * y;
          const double vx = V[p][j], vy = V[q][j];
          V[p][j] = c * vx - s * vy;
          V[q][j] = s * vx + c * vy;
        }
        I[p][p] = npp;
        I[q][q] = nqq;
        I[p][q] = I[q][p] = 0.0;
      }
  }
  int order[3] = {0, 1, 2};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (I[order[j + 1]][order[j + 1]] < I[order[j]][order[j]]) {
        const int tmp = order[j];
        order[j] = order[j + 1];
        order[j + 1] = tmp;
      }
  for (int k = 0; k < 3; ++k) {
    mom[k] = I[order[k]][order[k]];
    for (int j = 0; j < 3; ++j) ax[3 * k + j] = V[order[k]][j];
  }
}

struct VibProjectArgs {
  const void* hess;          // flat, graph g at hess_off[g]: [n, n, 3, 3]
  const int64_t* hess_off;   // [G]
  const double* pos;         // [N, 3]
  const double* mass;        // [N] amu
  const int64_t* ptr;        // [G + 1]
  int periodic;
  const int64_t* mat_off;    // [G]: graph g's [m, m] block of mat
  double* mat;
  double* q;                 // graph g at 18 ptr[g]: [6, m], rows n_tr .. 5 unused
  double* work;              // the same shape
  double* moments;           // [G, 3]
  double* axes;              // [G, 9]
  double* mass_tot;          // [G]
  int32_t* n_tr;             // [G]
  int32_t* rotor;            // [G]
  double* sigma;             // [G]
};

template <typename T>
__global__ void __launch_bounds__(VIB_THREADS) k_vib_project(VibProjectArgs a) {
  __shared__ double red[VIB_THREADS];
  __shared__ double sh_com[3], sh_ax[9], sh_C[36];
  __shared__ int sh_ntr, sh_first;
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int64_t b = a.ptr[g], n = a.ptr[g + 1] - b, m = 3 * n;
  if (n <= 0) {
    if (tid == 0) {
      a.n_tr[g] = 0;
      a.rotor[g] = XEQ_VIB_ATOM;
      a.mass_tot[g] = 0.0;
      a.sigma[g] = 0.0;
      for (int k = 0; k < 3; ++k) a.moments[3 * g + k] = 0.0;
      for (int k = 0; k < 9; ++k) a.axes[9 * g + k] = (k % 4 == 0) ? 1.0 : 0.0;
    }
    return;
  }
  const T* H = static_cast<const T*>(a.hess) + a.hess_off[g];
  const double* pos = a.pos + 3 * b;
  const double* mass = a.mass + b;
  double* M = a.mat + a.mat_off[g];
  double* Q = a.q + 18 * b;
  double* W = a.work + 18 * b;

  if (tid == 0) {
    double mt = 0.0, c[3] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i) {
      mt += mass[i];
      for (int k = 0; k < 3; ++k) c[k] += mass[i] * pos[3 * i + k];
    }
    for (int k = 0; k < 3; ++k) c[k] /= mt;
    double mom[3] = {0.0, 0.0, 0.0}, ax[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int rotor = n == 1 ? XEQ_VIB_ATOM : XEQ_VIB_NONLINEAR;
    if (!a.periodic && n > 1) {
      double I[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int64_t i = 0; i < n; ++i) {
        const double x = pos[3 * i] - c[0], y = pos[3 * i + 1] - c[1], z = pos[3 * i + 2] - c[2], w = mass[i];
        I[0][0] += w * (y * y + z * z);
        I[1][1] += w * (x * x + z * z);
        I[2][2] += w * (x * x + y * y);
        I[0][1] -= w * x * y;
        I[0][2] -= w * x * z;
        I[1][2] -= w * y * z;
      }
      I[1][0] = I[0][1];
      I[2][0] = I[0][2];
      I[2][1] = I[1][2];
      vib_jacobi3(I, mom, ax);
      if (mom[0] <= 1e-6 * mom[2]) rotor = XEQ_VIB_LINEAR;
    }
    const int ntr = (a.periodic || rotor == XEQ_VIB_ATOM) ? 3 : (rotor == XEQ_VIB_LINEAR ? 5 : 6);
    sh_ntr = ntr;
    sh_first = ntr == 5 ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
      sh_com[k] = c[k];
      a.moments[3 * g + k] = mom[k];
    }
    for (int k = 0; k < 9; ++k) {
      sh_ax[k] = ax[k];
      a.axes[9 * g + k] = ax[k];
    }
    a.mass_tot[g] = mt;
    a.n_tr[g] = ntr;
    a.rotor[g] = rotor;
  }
  __syncthreads();
  const int ntr = sh_ntr;

  // raw vectors; thread t owns the entries t, t + 256, ... of every vector until Q is complete
  for (int64_t e = tid; e < m; e += VIB_THREADS) {
    const int64_t i = e / 3;
    const int ax = (int)(e - 3 * i);
    const double sm = sqrt(mass[i]);
    for (int k = 0; k < 3; ++k) Q[k * m + e] = (ax == k) ? sm : 0.0;
    const double r[3] = {pos[3 * i] - sh_com[0], pos[3 * i + 1] - sh_com[1], pos[3 * i + 2] - sh_com[2]};
    for (int k = 3; k < ntr; ++k) {
      const double* u = &sh_ax[3 * (sh_first + k - 3)];
      const double cr[3] = {u[1] * r[2] - u[2] * r[1], u[2] * r[0] - u[0] * r[2], u[0] * r[1] - u[1] * r[0]};
      Q[k * m + e] = sm * cr[ax];
    }
  }
  // modified Gram-Schmidt, vectors in order
  for (int k = 0; k < ntr; ++k) {
    for (int j = 0; j < k; ++j) {
      double part = 0.0;
      for (int64_t e = tid; e < m; e += VIB_THREADS) part += Q[j * m + e] * Q[k * m + e];
      const double d = vib_block_sum(part, red);
      for (int64_t e = tid; e < m; e += VIB_THREADS) Q[k * m + e] -= d * Q[j * m + e];
    }
    double part = 0.0;
    for (int64_t e = tid; e < m; e += VIB_THREADS) part += Q[k * m + e] * Q[k * m + e];
    const double nrm = sqrt(vib_block_sum(part, red));
    const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
    for (int64_t e = tid; e < m; e += VIB_THREADS) Q[k * m + e] *= inv;
  }
  // S on the upper triangle, mirrored
  for (int64_t e = tid; e < m * m; e += VIB_THREADS) {
    const int64_t r = e / m, c = e - r * m;
    if (r > c) continue;
    const int64_t i = r / 3, k = c / 3;
    const int ar = (int)(r - 3 * i), ac = (int)(c - 3 * k);
    const double h1 = (double)H[((i * n + k) * 3 + ar) * 3 + ac], h2 = (double)H[((k * n + i) * 3 + ac) * 3 + ar];
    const double v = 0.5 * (h1 + h2) / (sqrt(mass[i]) * sqrt(mass[k]));
    M[r * m + c] = v;
    M[c * m + r] = v;
  }
  __syncthreads();
  // W = S Q (S is symmetric: column i read as row-major entries j m + i, consecutive threads on consecutive addresses)
  for (int64_t i = tid; i < m; i += VIB_THREADS) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t j = 0; j < m; ++j) {
      const double sji = M[j * m + i];
      for (int k = 0; k < 6; ++k)
        if (k < ntr) acc[k] += sji * Q[k * m + j];
    }
    for (int k = 0; k < ntr; ++k) W[k * m + i] = acc[k];
  }
  __syncthreads();
  if (tid < 36) {
    const int k = tid / 6, l = tid - 6 * k;
    if (k <= l && l < ntr) {
      double acc = 0.0;
      for (int64_t i = 0; i < m; ++i) acc += Q[k * m + i] * W[l * m + i];
      sh_C[6 * k + l] = acc;
      sh_C[6 * l + k] = acc;
    }
  }
  __syncthreads();
  // Y = W - Q C / 2, in place
  for (int64_t i = tid; i < m; i += VIB_THREADS) {
    double y[6];
    for (int k = 0; k < ntr; ++k) {
      double acc = 0.0;
      for (int l = 0; l < ntr; ++l) acc += sh_C[6 * k + l] * Q[l * m + i];
      y[k] = W[k * m + i] - 0.5 * acc;
    }
    for (int k = 0; k < ntr; ++k) W[k * m + i] = y[k];
  }
  __syncthreads();
  // P S P on the upper triangle, mirrored (the lower one is read by nobody), and its Frobenius norm
  double part = 0.0;
  for (int64_t e = tid; e < m * m; e += VIB_THREADS) {
    const int64_t r = e / m, c = e - r * m;
    if (r > c) continue;
    double v = M[r * m + c];
    for (int k = 0; k < ntr; ++k) v -= Q[k * m + r] * W[k * m + c] + W[k * m + r] * Q[k * m + c];
    M[r * m + c] = v;
    M[c * m + r] = v;
    part += (r == c ? 1.0 : 2.0) * (v * v);
  }
  double sig = 2.0 * sqrt(vib_block_sum(part, red));
  if (!(sig > 0.0) && sig == 0.0) sig = 1.0;
  for (int64_t e = tid; e < m * m; e += VIB_THREADS) {
    const int64_t r = e / m, c = e - r * m;
    if (r > c) continue;
    double qq = 0.0;
    for (int k = 0; k < ntr; ++k) qq += Q[k * m + r] * Q[k * m + c];
    const double v = M[r * m + c] + sig * qq;
    M[r * m + c] = v;
    M[c * m + r] = v;
  }
  if (tid == 0) a.sigma[g] = sig;
}

// ---- the eigensolver ---------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int vib_pairs(int m) { return (m + 1) >> 1; }
// bytes of dynamic LDS for matrices up to max_dim: A and V^T with the odd leading dimension, the rotation tables, the reduction scratch
__host__ __device__ inline size_t vib_eigh_lds_bytes(int max_dim) {
  const size_t ld = (size_t)(max_dim | 1), np = (size_t)vib_pairs(max_dim);
  return sizeof(double) * (2 * (size_t)max_dim * ld + 4 * np + VIB_THREADS) + sizeof(int) * 2 * np;
}

struct VibEighArgs {
  const double* mat;
  const int64_t* mat_off;   // [n]: matrix g (input) and its vectors (output)
  const int64_t* val_off;   // [n]: its eigenvalues
  const int32_t* dim;       // [n]
  int max_dim;              // what the LDS of the launch was sized for
  double* w;
  double* v;
  int32_t* sweeps;
  int32_t* status;
};

__global__ void __launch_bounds__(VIB_THREADS) k_vib_eigh(VibEighArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ve_lds[];
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int m = a.dim[g];
  if (m <= 0 || m > a.max_dim) {   // (the host checks the sizes before the launch: nothing is read or written beyond the tables)
    if (tid == 0) {
      a.sweeps[g] = 0;
      a.status[g] = m == 0 ? 0 : 2;
    }
    return;
  }
  const int ld = m | 1, mm = m + (m & 1), np = mm >> 1;
  double* A = ve_lds;                  // [m][ld]
  double* Vt = A + m * ld;             // [m][ld]  row k: vector k
  double* tc = Vt + m * ld;            // [np] each: c, s, new a_pp, new a_qq
  double* ts = tc + np;
  double* tpp = ts + np;
  double* tqq = tpp + np;
  double* red = tqq + np;              // [VIB_THREADS]
  int* tp = reinterpret_cast<int*>(red + VIB_THREADS);   // [np] p (-1: the pair rests), [np] q
  int* tq = tp + np;
  const uint32_t magic = (uint32_t)((1ull << 32) / (uint32_t)m) + 1u;   // e / m = umulhi(e, magic) for e m < 2^32
  const double* src = a.mat + a.mat_off[g];

  double part = 0.0;
  for (int e = tid; e < m * m; e += VIB_THREADS) {
    const int r = (int)__umulhi((uint32_t)e, magic), c = e - r * m;
    const double v = src[e];
    A[r * ld + c] = v;
    Vt[r * ld + c] = r == c ? 1.0 : 0.0;
    part += v * v;
  }
  const double tol = (double)m * 0x1p-53 * sqrt(vib_block_sum(part, red));

  int sweeps = 0, status = 0;
  while (true) {
    part = 0.0;
    for (int e = tid; e < m * m; e += VIB_THREADS) {
      const int r = (int)__umulhi((uint32_t)e, magic), c = e - r * m;
      const double v = A[r * ld + c];
      if (r != c) part += v * v;
    }
    const double off = sqrt(vib_block_sum(part, red));
    if (off <= tol) break;
    if (sweeps == XEQ_VIB_MAX_SWEEPS) {
      status = 1;
      break;
    }
    for (int s = 0; s < mm - 1; ++s) {
      if (tid < np) {
        int p, q;
        if (tid == 0) {
          p = mm - 1;
          q = s;
        } else {             // (s + tid) mod (mm - 1), (s - tid) mod (mm - 1): s < mm - 1, tid < mm / 2
          p = s + tid;
          if (p >= mm - 1) p -= mm - 1;
          q = s - tid;
          if (q < 0) q += mm - 1;
        }
        if (p > q) {
          const int x = p;
          p = q;
          q = x;
        }
        bool act = q < m;
        double c = 1.0, sn = 0.0, npp = 0.0, nqq = 0.0;
        if (act) {
          const double app = A[p * ld + p], aqq = A[q * ld + q], apq = A[p * ld + q];
          act = fabs(apq) > 0x1p-53 * sqrt(fabs(app * aqq));
          if (act) {
            double t;
            vib_rotation(app, aqq, apq, c, sn, t);
            npp = app - t * apq;
            nqq = aqq + t * apq;
          }
        }
        tp[tid] = act ? p : -1;
        tq[tid] = act ? q : 0;
        tc[tid] = c;
        ts[tid] = sn;
        tpp[tid] = npp;
        tqq[tid] = nqq;
      }
      __syncthreads();
      // The entries of one phase are disjoint, so VIB_BATCH of a thread's items are loaded before the first is stored: the LDS latencies of
      // a batch overlap instead of adding up (a step is latency-bound: one workgroup, a few entries per thread).
      const int items = np * m;
      for (int e0 = tid; e0 < items; e0 += VIB_THREADS * VIB_BATCH) {     // A <- A J: entries (i, p), (i, q)
        int ap[VIB_BATCH], aq[VIB_BATCH];
        double c[VIB_BATCH], sn[VIB_BATCH], x[VIB_BATCH], y[VIB_BATCH];
#pragma unroll
        for (int u = 0; u < VIB_BATCH; ++u) {
          const int e = e0 + u * VIB_THREADS, ee = e < items ? e : 0;
          const int k = (int)__umulhi((uint32_t)ee, magic), i = ee - k * m;
          const int p = tp[k], q = tq[k];
          const bool act = e < items && p >= 0;
          ap[u] = act ? i * ld + p : -1;
          aq[u] = i * ld + q;
          c[u] = tc[k];
          sn[u] = ts[k];
          x[u] = A[i * ld + (p < 0 ? 0 : p)];
          y[u] = A[aq[u]];
        }
#pragma unroll
        for (int u = 0; u < VIB_BATCH; ++u)
          if (ap[u] >= 0) {
            A[ap[u]] = c[u] * x[u] - sn[u] * y[u];
            A[aq[u]] = sn[u] * x[u] + c[u] * y[u];
          }
      }
      __syncthreads();
      for (int e0 = tid; e0 < items; e0 += VIB_THREADS * VIB_BATCH) {     // A <- J^T A, V^T <- J^T V^T: entries (p, j), (q, j)
        int ap[VIB_BATCH], aq[VIB_BATCH];
        double c[VIB_BATCH], sn[VIB_BATCH], x[VIB_BATCH], y[VIB_BATCH], vx[VIB_BATCH], vy[VIB_BATCH], dp[VIB_BATCH], dq[VIB_BATCH];
        int on[VIB_BATCH];     // 0: a plain entry, 1: column p, 2: column q
#pragma unroll
        for (int u = 0; u < VIB_BATCH; ++u) {
          const int e = e0 + u * VIB_THREADS, ee = e < items ? e : 0;
          const int k = (int)__umulhi((uint32_t)ee, magic), j = ee - k * m;
          const int p = tp[k], q = tq[k];
          const bool act = e < items && p >= 0;
          const int pp = p < 0 ? 0 : p;
          ap[u] = act ? pp * ld + j : -1;
          aq[u] = q * ld + j;
          on[u] = j == p ? 1 : (j == q ? 2 : 0);
          c[u] = tc[k];
          sn[u] = ts[k];
          dp[u] = tpp[k];
          dq[u] = tqq[k];
          x[u] = A[pp * ld + j];
          y[u] = A[aq[u]];
          vx[u] = Vt[pp * ld + j];
          vy[u] = Vt[aq[u]];
        }
#pragma unroll
        for (int u = 0; u < VIB_BATCH; ++u)
          if (ap[u] >= 0) {
            double nx = c[u] * x[u] - sn[u] * y[u], ny = sn[u] * x[u] + c[u] * y[u];
            if (on[u] == 1) {
              nx = dp[u];
              ny = 0.0;
            } else if (on[u] == 2) {
              nx = 0.0;
              ny = dq[u];
            }
            A[ap[u]] = nx;
            A[aq[u]] = ny;
            Vt[ap[u]] = c[u] * vx[u] - sn[u] * vy[u];
            Vt[aq[u]] = sn[u] * vx[u] + c[u] * vy[u];
          }
      }
      __syncthreads();
    }
    ++sweeps;
  }
  // rank of every diagonal entry (ascending, equal ones by index) and the sign of its vector; m <= 2 np <= the tables' 2 np ints / doubles
  int* rank = tp;        // [m] over tp | tq
  double* sgn = tc;      // [m] over tc | ts
  __syncthreads();
  if (tid < m) {
    const double d = A[tid * ld + tid];
    int r = 0;
    for (int j = 0; j < m; ++j) {
      const double dj = A[j * ld + j];
      r += (dj < d || (dj == d && j < tid)) ? 1 : 0;
    }
    double best = -1.0, at = 0.0;
    for (int j = 0; j < m; ++j) {
      const double v = Vt[tid * ld + j];
      if (fabs(v) > best) {
        best = fabs(v);
        at = v;
      }
    }
    rank[tid] = r;
    sgn[tid] = at < 0.0 ? -1.0 : 1.0;
    a.w[a.val_off[g] + r] = d;
  }
  __syncthreads();
  double* out = a.v + a.mat_off[g];
  for (int e = tid; e < m * m; e += VIB_THREADS) {
    const int k = (int)__umulhi((uint32_t)e, magic), j = e - k * m;
    out[rank[k] * m + j] = sgn[k] * Vt[k * ld + j];
  }
  if (tid == 0) {
    a.sweeps[g] = sweeps;
    a.status[g] = status;
  }
}

// ---- the eigensolver above the LDS cap ---------------------------------------------------------------------------------------------
// Smallest of one value per thread over the workgroup in a fixed tree; every thread gets it.  red: [VIB_THREADS] ints of LDS.
__device__ __forceinline__ int vib_block_min(int v, int* red) {
  const int t = threadIdx.x;
  __syncthreads();   // the previous result may still be being read
  red[t] = v;
  __syncthreads();
  for (int o = VIB_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = min(red[t], red[t + o]);
    __syncthreads();
  }
  return red[0];
}

// One workgroup per matrix, working in the matrix's own [m, m] block Z of the output (global memory, L2-resident; the barriers of a
// workgroup order its stores and loads as in k_vib_project); the tables d, e, u | c, p | s live in LDS.  Four phases:
//  1. Z <- A, then Householder reduction to tridiagonal form from the last row up.  Step i (m - 1 .. 1) works on the leading i x i block,
//     which is kept as a FULL symmetric matrix: x = row i (entries < i), sigma = sum_{k < i - 1} x_k^2 (the file's fixed pattern); sigma
//     == 0 (or not > 0: a NaN): no reflector, e_{i-1} = x_{i-1} + sigma.  Else g = -sign(x_{i-1}) sqrt(sigma + x_{i-1}^2), u = x with
//     u_{i-1} -= g, h = u.u / 2 = sigma + x_{i-1}^2 - x_{i-1} g, e_{i-1} = g; p = A u / h (thread r sums column r top to bottom:
//     coalesced, no reduction), K = u.p / 2h, q = p - K u, A -= u q^T + q u^T, entry (j, k) as fma(u_lo, q_hi, q_lo u_hi) with lo = min(j, k),
//     hi = max(j, k), so the block stays symmetric to the bit whatever the compiler contracts.  u stays in row i, h in Z[i][i] (d_i is in LDS).
//  2. Q = H_{m-1} .. H_1 accumulated in place from the top-left corner (step i: the i x i block <- H_i x it, thread j owns column j:
//     g_j = u.column / h, column -= g_j u; then row and column i of the block become those of the identity), then transposed in place:
//     row i of Z is column i of Q.
//  3. Implicit-shift QL on (d, e) with the running shift f (the EISPACK tql2 scheme): for l = 0 .. m - 1, tst1 = max(tst1, |d_l| + |e_l|);
//     per iteration every thread looks for the first k >= l with |e_k| <= 2^-52 tst1 (k = m - 1 when none: e_{m-1} is never read), a
//     fixed min tree; k == l: d_l + f is an eigenvalue.  Else lane 0 forms the shift and runs the (c, s) recurrence from k - 1 down to
//     l into LDS, one barrier, and thread r applies all rotations of the iteration to entry r of the rows k .. l, carrying the moving
//     row in a register.  (Every walk down the rows keeps several rows' loads in flight and a thread's up to three columns abreast:
//     the arithmetic and its order are those written here.)  Iteration XEQ_VIB_MAX_SWEEPS + 1 of one eigenvalue sets status 1 and leaves the loops; every loop is a
//     counted one, so a NaN (all comparisons false) ends there too; a non-finite eigenvalue gives status 1 as well.
//  4. Ranks (ascending, equal ones by index), signs (largest-magnitude component positive, lowest index on a tie), and the rows are
//     permuted in place along the permutation's cycles: thread r moves entry r of every row, lane 0 lists the cycles' first rows.
// sweeps: the largest iteration count of any eigenvalue.
constexpr int VIB_LARGE_DIM = XEQ_VIB_LARGE_MAX_DIM;
constexpr int VIB_ROWS = 8;      // rows of a column walk a thread has in flight: one workgroup per matrix is bound by the latency of its loads
static_assert(VIB_LARGE_DIM <= 3 * VIB_THREADS, "k_vib_eigh_large: a thread owns at most three columns");

// Thread t owns the columns t, t + 256, ... of the n leading ones (t < n, NC >= ceil(n / 256)).  A column beyond n is walked as the
// thread's first one and its result dropped, so that no load sits behind a branch.
template <int NC>
__device__ __forceinline__ void vib_columns(int n, int* col, bool* on) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int r = (int)threadIdx.x + c * VIB_THREADS;
    on[c] = r < n;
    col[c] = on[c] ? r : (int)threadIdx.x;
  }
}

// acc[c] = sum_k Z[k][col_c] t[k] over the rows k = 0 .. n - 1, top to bottom
template <int NC>
__device__ __forceinline__ void vib_column_dots(const double* Z, int m, int n, const int* col, const double* t, double* acc) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  int k = 0;
  for (; k + VIB_ROWS <= n; k += VIB_ROWS) {
    double z[VIB_ROWS][NC];
#pragma unroll
    for (int u = 0; u < VIB_ROWS; ++u)
#pragma unroll
      for (int c = 0; c < NC; ++c) z[u][c] = Z[(k + u) * m + col[c]];
#pragma unroll
    for (int u = 0; u < VIB_ROWS; ++u) {
      const double tk = t[k + u];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] += z[u][c] * tk;
    }
  }
  for (; k < n; ++k) {
    const double tk = t[k];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += Z[k * m + col[c]] * tk;
  }
}

// Reduction step on the leading i x i block: p_r = (A u)_r / h into tp for the thread's columns; returns its part of u.p
template <int NC>
__device__ __forceinline__ double vib_reduce_products(const double* Z, int m, int i, double hh, const double* tu, double* tp) {
  if ((int)threadIdx.x >= i) return 0.0;
  int col[NC];
  bool on[NC];
  double acc[NC];
  vib_columns<NC>(i, col, on);
  vib_column_dots<NC>(Z, m, i, col, tu, acc);
  double part = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (on[c]) {
      const double pr = acc[c] / hh;
      tp[col[c]] = pr;
      part += tu[col[c]] * pr;
    }
  return part;
}

// Accumulation step: the leading i x i block <- (I - u u^T / h) x it, a thread on its own columns
template <int NC>
__device__ __forceinline__ void vib_reflect_columns(double* Z, int m, int i, double hh, const double* tu) {
  if ((int)threadIdx.x >= i) return;
  int col[NC];
  bool on[NC];
  double acc[NC];
  vib_columns<NC>(i, col, on);
  vib_column_dots<NC>(Z, m, i, col, tu, acc);
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] /= hh;
  int k = 0;
  for (; k + VIB_ROWS <= i; k += VIB_ROWS) {
    double z[VIB_ROWS][NC];
#pragma unroll
    for (int u = 0; u < VIB_ROWS; ++u)
#pragma unroll
      for (int c = 0; c < NC; ++c) z[u][c] = Z[(k + u) * m + col[c]];
#pragma unroll
    for (int u = 0; u < VIB_ROWS; ++u) {
      const double tk = tu[k + u];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (on[c]) Z[(k + u) * m + col[c]] = z[u][c] - acc[c] * tk;
    }
  }
  for (; k < i; ++k) {
    const double tk = tu[k];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (on[c]) Z[k * m + col[c]] -= acc[c] * tk;
  }
}

// One QL iteration's rotations (c_i, s_i), i = mm - 1 .. l, on the rows i, i + 1 of Q^T: a thread on its own columns, the moving row
// in a register, the loads of four rows ahead of the stores
template <int NC>
__device__ __forceinline__ void vib_rotate_rows(double* Z, int m, int l, int mm, const double* tc, const double* ts) {
  if ((int)threadIdx.x >= m) return;
  int col[NC];
  bool on[NC];
  double carry[NC];
  vib_columns<NC>(m, col, on);
#pragma unroll
  for (int c = 0; c < NC; ++c) carry[c] = Z[mm * m + col[c]];
  int i = mm - 1;
  for (; i - 3 >= l; i -= 4) {
    double z[4][NC];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < NC; ++c) z[u][c] = Z[(i - u) * m + col[c]];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double cs = tc[i - u], sn = ts[i - u];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double out = sn * z[u][c] + cs * carry[c];
        carry[c] = cs * z[u][c] - sn * carry[c];
        if (on[c]) Z[(i - u + 1) * m + col[c]] = out;
      }
    }
  }
  for (; i >= l; --i) {
    const double cs = tc[i], sn = ts[i];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double z0 = Z[i * m + col[c]];
      const double out = sn * z0 + cs * carry[c];
      carry[c] = cs * z0 - sn * carry[c];
      if (on[c]) Z[(i + 1) * m + col[c]] = out;
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (on[c]) Z[l * m + col[c]] = carry[c];
}

__global__ void __launch_bounds__(VIB_THREADS) k_vib_eigh_large(VibEighArgs a) {
  __shared__ double td[VIB_LARGE_DIM], te[VIB_LARGE_DIM], tu[VIB_LARGE_DIM], tp[VIB_LARGE_DIM];
  __shared__ double red[VIB_THREADS];
  __shared__ int redi[VIB_THREADS], trank[VIB_LARGE_DIM], tlead[VIB_LARGE_DIM];
  __shared__ double sh_h;
  __shared__ int sh_n;
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int m = a.dim[g];
  if (m <= 0 || m > a.max_dim || m > VIB_LARGE_DIM) {   // (the host checks the sizes before the launch: nothing is read or written beyond the tables)
    if (tid == 0) {
      a.sweeps[g] = 0;
      a.status[g] = m == 0 ? 0 : 2;
    }
    return;
  }
  const double* src = a.mat + a.mat_off[g];
  double* Z = a.v + a.mat_off[g];
  for (int e = tid; e < m * m; e += VIB_THREADS) Z[e] = src[e];
  __syncthreads();

  // 1. reduction
  for (int i = m - 1; i >= 1; --i) {
    double* row = Z + i * m;
    double part = 0.0;
    for (int k = tid; k < i; k += VIB_THREADS) {
      const double x = row[k];
      tu[k] = x;
      if (k < i - 1) part += x * x;
    }
    const double sigma = vib_block_sum(part, red);
    const double f = tu[i - 1];
    if (!(sigma > 0.0)) {
      if (tid == 0) {
        td[i] = row[i];
        te[i - 1] = f + sigma;     // sigma is 0, or a NaN that must not be lost
        row[i] = 0.0;
      }
      continue;     // (the next step writes tu below i - 1 only, and red behind a barrier)
    }
    const double nrm2 = sigma + f * f;
    const double gg = -copysign(sqrt(nrm2), f);
    const double hh = nrm2 - f * gg;
    __syncthreads();     // every thread has read tu[i - 1]
    if (tid == 0) {
      td[i] = row[i];
      te[i - 1] = gg;
      tu[i - 1] = f - gg;
      row[i - 1] = f - gg;
      row[i] = hh;
    }
    __syncthreads();
    part = i <= VIB_THREADS ? vib_reduce_products<1>(Z, m, i, hh, tu, tp)
                            : (i <= 2 * VIB_THREADS ? vib_reduce_products<2>(Z, m, i, hh, tu, tp) : vib_reduce_products<3>(Z, m, i, hh, tu, tp));
    const double kk = vib_block_sum(part, red) / (2.0 * hh);
    for (int r = tid; r < i; r += VIB_THREADS) tp[r] -= kk * tu[r];
    __syncthreads();
    const uint32_t magic = (uint32_t)((1ull << 32) / (uint32_t)i) + 1u;   // e / i = umulhi(e, magic) for e i < 2^32; i >= 2 here
    for (int e0 = tid; e0 < i * i; e0 += VIB_THREADS * VIB_BATCH) {
      int at[VIB_BATCH];
      double z[VIB_BATCH];
#pragma unroll
      for (int u = 0; u < VIB_BATCH; ++u) {
        const int e = e0 + u * VIB_THREADS, ee = e < i * i ? e : 0;
        const int j = (int)__umulhi((uint32_t)ee, magic), k = ee - j * i;
        const int lo = min(j, k), hi = max(j, k);
        at[u] = e < i * i ? j * m + k : -1;
        z[u] = Z[j * m + k] - fma(tu[lo], tp[hi], tp[lo] * tu[hi]);
      }
#pragma unroll
      for (int u = 0; u < VIB_BATCH; ++u)
        if (at[u] >= 0) Z[at[u]] = z[u];
    }
    __syncthreads();
  }
  if (tid == 0) {
    td[0] = Z[0];
    te[m - 1] = 0.0;
    Z[0] = 1.0;
  }
  __syncthreads();

  // 2. Q, then Q^T
  for (int i = 1; i < m; ++i) {
    double* row = Z + i * m;
    const double hh = row[i];
    if (hh > 0.0) {
      for (int k = tid; k < i; k += VIB_THREADS) tu[k] = row[k];
      __syncthreads();
      if (i <= VIB_THREADS) vib_reflect_columns<1>(Z, m, i, hh, tu);
      else if (i <= 2 * VIB_THREADS) vib_reflect_columns<2>(Z, m, i, hh, tu);
      else vib_reflect_columns<3>(Z, m, i, hh, tu);
    }
    __syncthreads();     // h and u have been read, the columns are complete
    for (int k = tid; k < i; k += VIB_THREADS) {
      row[k] = 0.0;
      Z[k * m + i] = 0.0;
    }
    if (tid == 0) row[i] = 1.0;
    __syncthreads();
  }
  if (m > 1) {
    const uint32_t magic = (uint32_t)((1ull << 32) / (uint32_t)m) + 1u;
    for (int e = tid; e < m * m; e += VIB_THREADS) {
      const int r = (int)__umulhi((uint32_t)e, magic), c = e - r * m;
      if (r < c) {
        const double x = Z[r * m + c], y = Z[c * m + r];
        Z[r * m + c] = y;
        Z[c * m + r] = x;
      }
    }
  }
  __syncthreads();

  // 3. QL
  int sweeps = 0, status = 0;
  double fshift = 0.0, tst1 = 0.0;
  for (int l = 0; l < m && status == 0; ++l) {
    tst1 = fmax(tst1, fabs(td[l]) + fabs(te[l]));
    int iter = 0;
    while (true) {     // at most XEQ_VIB_MAX_SWEEPS + 1 passes: a pass ends the loop or counts one iteration
      const double thr = 0x1p-52 * tst1;
      int cand = m - 1;
      for (int k = l + tid; k < m - 1; k += VIB_THREADS)
        if (fabs(te[k]) <= thr) {
          cand = k;
          break;
        }
      const int mm = vib_block_min(cand, redi);
      if (mm == l) break;
      if (iter == XEQ_VIB_MAX_SWEEPS) {
        status = 1;
        break;
      }
      ++iter;
      if (tid == 0) {
        const double el = te[l], g0 = td[l], el1 = te[l + 1];
        double p = (td[l + 1] - g0) / (2.0 * el);
        double r = hypot(p, 1.0);
        const double pr = p + copysign(r, p);
        const double dl = el / pr, dl1 = el * pr, h = g0 - dl;
        td[l] = dl;
        td[l + 1] = dl1;
        p = mm >= l + 2 ? td[mm] - h : td[mm];     // the entries l + 2 .. mm take the shift as they are read, those above mm below
        double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
        for (int i = mm - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          const double ei = te[i], di = i >= l + 2 ? td[i] - h : td[i];
          const double ce = c * ei, cp = c * p;
          r = hypot(p, ei);
          te[i + 1] = s * r;
          s = ei / r;
          c = p / r;
          p = c * di - s * ce;
          td[i + 1] = cp + s * (c * ce + s * di);
          tu[i] = c;
          tp[i] = s;
        }
        p = -s * s2 * c3 * el1 * el / dl1;
        te[l] = s * p;
        td[l] = c * p;
        sh_h = h;
      }
      __syncthreads();
      const double h = sh_h;
      fshift += h;
      for (int k = mm + 1 + tid; k < m; k += VIB_THREADS) td[k] -= h;
      if (m <= VIB_THREADS) vib_rotate_rows<1>(Z, m, l, mm, tu, tp);
      else if (m <= 2 * VIB_THREADS) vib_rotate_rows<2>(Z, m, l, mm, tu, tp);
      else vib_rotate_rows<3>(Z, m, l, mm, tu, tp);
      __syncthreads();
    }
    sweeps = max(sweeps, iter);
    if (tid == 0) td[l] += fshift;
  }

  // 4. order, signs, output
  __syncthreads();     // lane 0's last d_l + f
  double bad = 0.0;
  for (int k = tid; k < m; k += VIB_THREADS)
    if (!isfinite(td[k])) bad = 1.0;
  if (vib_block_sum(bad, red) > 0.0) status = 1;
  double* sgn = tu;       // [m]
  double* seen = tp;      // [m]
  for (int k = tid; k < m; k += VIB_THREADS) {
    const double d = td[k];
    int r = 0;
    for (int j = 0; j < m; ++j) {
      const double dj = td[j];
      r += (dj < d || (dj == d && j < k)) ? 1 : 0;
    }
    double best = -1.0, at = 0.0;
    for (int j0 = 0; j0 < m; j0 += VIB_ROWS) {
      double v[VIB_ROWS];
#pragma unroll
      for (int u = 0; u < VIB_ROWS; ++u) v[u] = Z[k * m + min(j0 + u, m - 1)];     // (the last entry again: never larger than itself)
#pragma unroll
      for (int u = 0; u < VIB_ROWS; ++u)
        if (fabs(v[u]) > best) {
          best = fabs(v[u]);
          at = v[u];
        }
    }
    if (status != 0) r = k;     // not a spectrum: the rows stay where they are
    trank[k] = r;
    sgn[k] = at < 0.0 ? -1.0 : 1.0;
    seen[k] = 0.0;
    a.w[a.val_off[g] + r] = d;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < m; ++k) {
      if (seen[k] != 0.0) continue;
      tlead[n++] = k;
      int j = k;
      for (int c = 0; c < m && seen[j] == 0.0; ++c) {
        seen[j] = 1.0;
        j = trank[j];
      }
    }
    sh_n = n;
  }
  __syncthreads();
  const int n_cycles = sh_n;
  for (int c = tid; c < m; c += VIB_THREADS)
    for (int q = 0; q < n_cycles; ++q) {
      const int k0 = tlead[q];
      int j = k0;
      double val = sgn[j] * Z[j * m + c];     // row j, on its way to row trank[j]
      for (int n = 0; n < m; ++n) {
        const int t = trank[j];
        if (t == k0) {
          Z[k0 * m + c] = val;
          break;
        }
        const double next = sgn[t] * Z[t * m + c];
        Z[t * m + c] = val;
        val = next;
        j = t;
      }
    }
  if (tid == 0) {
    a.sweeps[g] = sweeps;
    a.status[g] = status;
  }
}

// ---- modes, frequencies, thermochemistry sums --------------------------------------------------------------------------------------
struct VibFinishArgs {
  const double* w;           // eigenvalues, graph g at 3 ptr[g]
  const double* v;           // vectors, graph g at mat_off[g]: [m, m]
  const int64_t* mat_off;
  const double* mass;
  const int64_t* ptr;
  const int32_t* n_tr;
  const int64_t* mode_ptr;   // [G + 1]: sum of m - n_tr
  const int64_t* mode_off;   // [G]: sum of (m - n_tr) m
  double to_wavenumber, to_kelvin;
  double* eigenvalue;
  double* norm_mode;
  double* reduced_mass;
  double* freq;
  double* vib_temperature;
  double* force_const;
  int32_t* n_imaginary;
};

__global__ void __launch_bounds__(VIB_THREADS) k_vib_finish(VibFinishArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int64_t b = a.ptr[g], n = a.ptr[g + 1] - b, m = 3 * n;
  const int64_t nk = m - a.n_tr[g];
  const double* w = a.w + 3 * b;
  if (tid == 0) {
    int cnt = 0;
    for (int64_t k = 0; k < nk; ++k) cnt += w[k] < 0.0 ? 1 : 0;
    a.n_imaginary[g] = cnt;
  }
  if (nk <= 0) return;
  const double* v = a.v + a.mat_off[g];
  const double* mass = a.mass + b;
  const int64_t k0 = a.mode_ptr[g];
  double* nm = a.norm_mode + a.mode_off[g];
  for (int64_t k = wave; k < nk; k += VIB_THREADS / 64) {
    double part = 0.0;
    for (int64_t e = lane; e < m; e += 64) {
      const double x = v[k * m + e] / sqrt(mass[e / 3]);
      nm[k * m + e] = x;
      part += x * x;
    }
    const double total = wave_sum(part);
    if (lane == 0) {
      const double lam = w[k], root = sqrt(fabs(lam)), sg = lam < 0.0 ? -1.0 : 1.0;
      const double rm = 1.0 / total;
      a.eigenvalue[k0 + k] = lam;
      a.reduced_mass[k0 + k] = rm;
      a.freq[k0 + k] = sg * root * a.to_wavenumber;
      a.vib_temperature[k0 + k] = sg * root * a.to_kelvin;
      a.force_const[k0 + k] = rm * lam;
    }
  }
}

// sums [G, 4] over the modes with lambda > 0, x = theta / T: theta / 2 | theta / (e^x - 1) | x / (e^x - 1) - ln(1 - e^-x) |
// x^2 e^x / (e^x - 1)^2, written with e^-x so that a large x underflows to the right limit instead of overflowing
__global__ void __launch_bounds__(64) k_vib_thermo_sums(const double* theta, const double* lam, const int64_t* mode_ptr, double T, double* sums) {
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t k = mode_ptr[g] + lane; k < mode_ptr[g + 1]; k += 64) {
    if (!(lam[k] > 0.0)) continue;
    const double th = theta[k], x = th / T;
    const double em = exp(-x), d = -expm1(-x);   // e^-x, 1 - e^-x
    s[0] += 0.5 * th;
    s[1] += th * em / d;
    s[2] += x * em / d - log1p(-em);
    s[3] += x * x * em / (d * d);
  }
  for (int c = 0; c < 4; ++c) {
    const double total = wave_sum(s[c]);
    if (lane == 0) sums[4 * g + c] = total;
  }
}

}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_vib_project(int dtype, const void* hess, const int64_t* hess_off, const double* pos, const double* mass, const int64_t* ptr,
                    int64_t n_graphs, int periodic, const int64_t* mat_off, double* mat, double* q, double* work, double* moments, double* axes,
                    double* mass_tot, int32_t* n_tr, int32_t* rotor, double* sigma, void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_vib_project: dtype %d", dtype);
  XEQ_CHECK_ARG(n_graphs >= 0 && n_graphs <= 0x7fffffff, "xeq_vib_project: n_graphs %lld", (long long)n_graphs);
  XEQ_CHECK_ARG(n_graphs == 0 || (hess_off && pos && mass && ptr && mat_off && moments && axes && mass_tot && n_tr && rotor && sigma),
                "xeq_vib_project: null buffer");
  if (n_graphs == 0) return XEQ_OK;
  VibProjectArgs a{hess, hess_off, pos, mass, ptr, periodic ? 1 : 0, mat_off, mat, q, work, moments, axes, mass_tot, n_tr, rotor, sigma};
  if (dtype == XEQ_F32) hipLaunchKernelGGL(k_vib_project<float>, dim3((unsigned)n_graphs), dim3(VIB_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_vib_project<double>, dim3((unsigned)n_graphs), dim3(VIB_THREADS), 0, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_vib_project");
  return XEQ_OK;
}

int xeq_vib_eigh(const double* mat, const int64_t* mat_off, const int64_t* val_off, const int32_t* dim, int64_t n, int max_dim,
                 double* eigenvalues, double* eigenvectors, int32_t* sweeps, int32_t* status, void* stream) {
  XEQ_CHECK_ARG(max_dim >= 0 && max_dim <= XEQ_VIB_MAX_DIM,
                "xeq_vib_eigh: dimension %d is beyond XEQ_VIB_MAX_DIM = %d (A and V do not fit the LDS of a compute unit)", max_dim, XEQ_VIB_MAX_DIM);
  XEQ_CHECK_ARG(n >= 0 && n <= 0x7fffffff, "xeq_vib_eigh: n %lld", (long long)n);
  XEQ_CHECK_ARG(n == 0 || (mat_off && val_off && dim && sweeps && status), "xeq_vib_eigh: null buffer");
  XEQ_CHECK_ARG(n == 0 || max_dim == 0 || (mat && eigenvalues && eigenvectors), "xeq_vib_eigh: null matrix buffer");
  if (n == 0) return XEQ_OK;
  const size_t shmem = vib_eigh_lds_bytes(max_dim);
  static const hipError_t lds_err = raise_dynamic_lds({reinterpret_cast<const void*>(&k_vib_eigh)}, vib_eigh_lds_bytes(XEQ_VIB_MAX_DIM));
  XEQ_CHECK_ARG(lds_err == hipSuccess, "xeq_vib_eigh: cannot raise the dynamic LDS limit");
  VibEighArgs a{mat, mat_off, val_off, dim, max_dim, eigenvalues, eigenvectors, sweeps, status};
  hipLaunchKernelGGL(k_vib_eigh, dim3((unsigned)n), dim3(VIB_THREADS), shmem, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_vib_eigh");
  return XEQ_OK;
}

int xeq_vib_eigh_large(const double* mat, const int64_t* mat_off, const int64_t* val_off, const int32_t* dim, int64_t n, int max_dim,
                       double* eigenvalues, double* eigenvectors, int32_t* sweeps, int32_t* status, void* stream) {
  XEQ_CHECK_ARG(max_dim >= 0 && max_dim <= XEQ_VIB_LARGE_MAX_DIM,
                "xeq_vib_eigh_large: dimension %d is beyond XEQ_VIB_LARGE_MAX_DIM = %d (one workgroup per matrix is the wrong shape above it)", max_dim,
                XEQ_VIB_LARGE_MAX_DIM);
  XEQ_CHECK_ARG(n >= 0 && n <= 0x7fffffff, "xeq_vib_eigh_large: n %lld", (long long)n);
  XEQ_CHECK_ARG(n == 0 || (mat_off && val_off && dim && sweeps && status), "xeq_vib_eigh_large: null buffer");
  XEQ_CHECK_ARG(n == 0 || max_dim == 0 || (mat && eigenvalues && eigenvectors), "xeq_vib_eigh_large: null matrix buffer");
  if (n == 0) return XEQ_OK;
  VibEighArgs a{mat, mat_off, val_off, dim, max_dim, eigenvalues, eigenvectors, sweeps, status};
  hipLaunchKernelGGL(k_vib_eigh_large, dim3((unsigned)n), dim3(VIB_THREADS), 0, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_vib_eigh_large");
  return XEQ_OK;
}

int xeq_vib_finish(const double* eigenvalues, const double* eigenvectors, const int64_t* mat_off, const double* mass, const int64_t* ptr,
                   int64_t n_graphs, const int32_t* n_tr, const int64_t* mode_ptr, const int64_t* mode_off, double to_wavenumber, double to_kelvin,
                   double* eigenvalue, double* norm_mode, double* reduced_mass, double* freq_wavenumber, double* vib_temperature,
                   double* force_const, int32_t* n_imaginary, void* stream) {
  XEQ_CHECK_ARG(n_graphs >= 0 && n_graphs <= 0x7fffffff, "xeq_vib_finish: n_graphs %lld", (long long)n_graphs);
  XEQ_CHECK_ARG(n_graphs == 0 || (mat_off && mass && ptr && n_tr && mode_ptr && mode_off && n_imaginary), "xeq_vib_finish: null buffer");
  if (n_graphs == 0) return XEQ_OK;
  VibFinishArgs a{eigenvalues, eigenvectors, mat_off, mass, ptr, n_tr, mode_ptr, mode_off, to_wavenumber, to_kelvin, eigenvalue, norm_mode,
                  reduced_mass, freq_wavenumber, vib_temperature, force_const, n_imaginary};
  hipLaunchKernelGGL(k_vib_finish, dim3((unsigned)n_graphs), dim3(VIB_THREADS), 0, (hipStream_t)stream, a);
  XEQ_CHECK_LAUNCH("xeq_vib_finish");
  return XEQ_OK;
}

int xeq_vib_thermo_sums(const double* vib_temperature, const double* eigenvalue, const int64_t* mode_ptr, int64_t n_graphs, double temperature,
                        double* sums, void* stream) {
  XEQ_CHECK_ARG(n_graphs >= 0 && n_graphs <= 0x7fffffff, "xeq_vib_thermo_sums: n_graphs %lld", (long long)n_graphs);
  XEQ_CHECK_ARG(temperature > 0.0, "xeq_vib_thermo_sums: temperature %g K", temperature);
  XEQ_CHECK_ARG(n_graphs == 0 || (mode_ptr && sums), "xeq_vib_thermo_sums: null buffer");
  if (n_graphs == 0) return XEQ_OK;
  hipLaunchKernelGGL(k_vib_thermo_sums, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream, vib_temperature, eigenvalue, mode_ptr,
                     temperature, sums);
  XEQ_CHECK_LAUNCH("xeq_vib_thermo_sums");
  return XEQ_OK;
}

}  // extern "C"
