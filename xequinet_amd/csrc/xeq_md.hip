// Device-resident molecular dynamics around the whole-step graphs (xequinet_amd/md.py): the integrator's two
// halves -- xeq_md_front in front of the step's graph, xeq_md_back behind it -- and the counter-based generator they share with
// xeq_md_normals.  Plain vector code, f32 and f64 state.
//
// Arithmetic.  Every per-atom update is evaluated in double whatever the state's type and rounded ONCE when it is stored: the state of an
// f32 run is within half an ulp of the f64 value of the same expression on the same stored inputs, and no result depends on how the compiler
// would have contracted an f32 chain.  The file is built with -ffp-contract=off (csrc/build.py), so the double expressions are the ones
// written here, operation by operation (tests/md_oracle.py restates them in numpy).  The generator's transcendentals run in the state's own type (logf / sincosf for
// f32, log / sincos for f64); its integers are exact.
//
// Sums.  A graph's kinetic energy is formed from partial sums over chunks of MD_CHUNK atoms COUNTED FROM THE GRAPH'S FIRST ATOM (one
// workgroup per chunk: lanes, then a butterfly, then the four waves in order), joined in chunk order (k_md_join): no float atomic, and the
// order depends on the graph's own atom count alone, so a graph has the same bits alone and anywhere in a batch.
#include "xeq_common.h"

namespace xeq {

constexpr int MD_CHUNK = XEQ_MD_CHUNK;
constexpr int MD_JOIN_THREADS = 1024;
constexpr int MD_JOIN_SERIAL = 4;   // chunks one lane adds by itself

// ------------------------------------------------------------------------------------------------------------- generator
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The block of (seed, purpose, id, step): the layout documented at xeq_md_normals in include/xeq.h.
__host__ __device__ __forceinline__ void md_block(uint64_t seed, int purpose, int64_t id, uint64_t step, uint32_t w[4]) {
  w[0] = (uint32_t)(uint64_t)id;
  w[1] = (uint32_t)((uint64_t)id >> 32);
  w[2] = (uint32_t)step;
  w[3] = (uint32_t)(step >> 32) | ((uint32_t)purpose << 30);
  philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Three normals from the four words by Box-Muller: u = (x + 1) 2^-32 in (0, 1], formed exactly in double and rounded once to T.
template <typename T>
__device__ __forceinline__ void md_normals3(const uint32_t w[4], T out[3]) {
  const double s = 2.3283064365386962890625e-10;   // 2^-32
  const T u0 = (T)(((double)w[0] + 1.0) * s), u1 = (T)(((double)w[1] + 1.0) * s);
  const T u2 = (T)(((double)w[2] + 1.0) * s), u3 = (T)(((double)w[3] + 1.0) * s);
  const T two_pi = (T)6.283185307179586476925286766559;
  T sn, cs;
  const T r0 = sqrt_<T>(T(-2) * log_<T>(u0));
  sincos_<T>(two_pi * u1, &sn, &cs);
  out[0] = r0 * cs;
  out[1] = r0 * sn;
  const T r1 = sqrt_<T>(T(-2) * log_<T>(u2));
  sincos_<T>(two_pi * u3, &sn, &cs);
  out[2] = r1 * cs;
}

template <typename T>
__global__ void __launch_bounds__(256) k_md_normals(uint64_t seed, int purpose, uint64_t step, const int64_t* __restrict__ id, int64_t n,
                                                    uint32_t* __restrict__ words, T* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4];
  md_block(seed, purpose, id[i], step, w);
  if (words) {
    for (int k = 0; k < 4; ++k) words[4 * i + k] = w[k];
  }
  if (normals) {
    T z[3];
    md_normals3<T>(w, z);
    for (int k = 0; k < 3; ++k) normals[3 * i + k] = z[k];
  }
}

// ------------------------------------------------------------------------------------------------------------- front
struct MdBox {
  double cell[9];   // rows: lattice vectors
  double inv[9];    // frac_k = sum_j x_j inv[3 j + k]
  int periodic[3];
  int any;
};

template <typename T>
struct MdFrontArgs {
  int64_t n, n_graphs;
  int ensemble;
  T* pos;
  T* vel;
  const T* frc;
  const T* inv_mass;
  const int64_t* batch;
  const T* ke;
  const T* tfac;
  const int64_t* rng_id;
  const int64_t* book;
  uint64_t seed;
  double dt, c1, noise2, dt_over_tau, t0;
  int32_t* image;
  MdBox box;
};

// Fractional coordinate by the inverse cell, floor, subtract along the periodic axes; twice, because the rounding of the wrapped coordinate
// to T can land an atom that was a hair below a face exactly ON the opposite face.
template <typename T>
__device__ __forceinline__ void md_wrap(const MdBox& b, double x[3], int32_t img[3]) {
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = 0; k < 3; ++k) x[k] = (double)(T)x[k];
    double s[3];
    for (int k = 0; k < 3; ++k) {
      const double fr = (x[0] * b.inv[k] + x[1] * b.inv[3 + k]) + x[2] * b.inv[6 + k];
      s[k] = b.periodic[k] ? floor(fr) : 0.0;
    }
    for (int j = 0; j < 3; ++j) x[j] = x[j] - ((s[0] * b.cell[j] + s[1] * b.cell[3 + j]) + s[2] * b.cell[6 + j]);
    for (int k = 0; k < 3; ++k) img[k] += (int32_t)s[k];
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_md_front(MdFrontArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double im = (double)a.inv_mass[i];
  double v[3], x[3], f[3];
  for (int k = 0; k < 3; ++k) {
    v[k] = (double)a.vel[3 * i + k];
    x[k] = (double)a.pos[3 * i + k];
    f[k] = (double)a.frc[3 * i + k];
  }
  if (a.ensemble == XEQ_MD_BERENDSEN) {
    int64_t g = a.batch[i];
    g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);
    const double tg = (double)a.ke[g] * (double)a.tfac[g];
    double lam = 1.0;
    if (tg > 0.0) {
      lam = sqrt(1.0 + a.dt_over_tau * (a.t0 / tg - 1.0));
      lam = fmin(fmax(lam, 0.9), 1.1);
    }
    for (int k = 0; k < 3; ++k) v[k] = lam * v[k];
  }
  const double h = 0.5 * a.dt;
  if (im > 0.0) {   // (a fixed atom keeps its position and a zero velocity whatever its force holds)
    for (int k = 0; k < 3; ++k) v[k] = v[k] + h * (f[k] * im);
    if (a.ensemble == XEQ_MD_LANGEVIN) {
      // A(1/2) O A(1/2): nothing reads the position between the two half drifts, so they are one update by h (v + v'), which at
      // c1 = 1 is the plain drift dt v bit for bit
      uint32_t w[4];
      md_block(a.seed, XEQ_MD_PURPOSE_LANGEVIN, a.rng_id[i], (uint64_t)a.book[0], w);
      T z[3];
      md_normals3<T>(w, z);
      const double sigma = sqrt(a.noise2 * im);
      for (int k = 0; k < 3; ++k) {
        const double vn = a.c1 * v[k] + sigma * (double)z[k];
        x[k] = x[k] + h * (v[k] + vn);
        v[k] = vn;
      }
    } else {
      for (int k = 0; k < 3; ++k) x[k] = x[k] + a.dt * v[k];
    }
  } else {
    for (int k = 0; k < 3; ++k) v[k] = 0.0;
  }
  if (a.box.any) {
    int32_t img[3] = {a.image[3 * i], a.image[3 * i + 1], a.image[3 * i + 2]};
    md_wrap<T>(a.box, x, img);
    for (int k = 0; k < 3; ++k) a.image[3 * i + k] = img[k];
  }
  for (int k = 0; k < 3; ++k) {
    a.vel[3 * i + k] = (T)v[k];
    a.pos[3 * i + k] = (T)x[k];
  }
}

// ------------------------------------------------------------------------------------------------------------- back
template <typename T>
struct MdBackArgs {
  int64_t n, n_graphs, n_chunks;
  int advance;
  const T* pos;
  T* vel;
  T* frc;
  const T* frc_step;
  const T* energy_step;
  const int32_t* n_edges_step;
  const T* inv_mass;
  const T* half_mass;
  const int32_t* chunk_atom0;
  const int32_t* chunk_n;
  const int32_t* graph_chunk_ptr;
  double* partial;
  int32_t* partial_bad;
  T* ke;
  T* epot;
  int64_t* book;
  double half_dt;
  const int32_t* image;
  MdBox box;
  int64_t record_every, record_start, record_rows;
  T* traj_pos;
  T* traj_epot;
  T* traj_ekin;
  int64_t* traj_step;
};

// The trajectory row this step fills (-1: none): row (step - record_start) / record_every - 1 of the run's buffers, `step` counted behind it.
template <typename T>
__device__ __forceinline__ int64_t md_record_row(const MdBackArgs<T>& a, int64_t step_after) {
  if (!a.advance || a.record_every <= 0) return -1;
  const int64_t d = step_after - a.record_start;
  if (d <= 0 || d % a.record_every) return -1;
  const int64_t row = d / a.record_every - 1;
  return row < a.record_rows ? row : -1;
}

__device__ __forceinline__ double md_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// One workgroup joins every graph's chunk partials in chunk order; then ONE lane does the bookkeeping with plain stores.  A graph of at
// most MD_JOIN_SERIAL chunks is summed by one lane, chunk after chunk (a batch of many small molecules: a graph per lane); a larger one by
// a wave, lane l adding chunks l, l + 64, ... and a butterfly.  Which of the two depends on the graph's own chunk count alone.
template <typename T>
__device__ __forceinline__ void md_join_store(const MdBackArgs<T>& a, int64_t g, int64_t row, double s, int* bad) {
  const T e = a.energy_step[g];
  *bad |= !isfinite((double)e);
  a.ke[g] = (T)s;
  a.epot[g] = e;
  if (row >= 0) {
    a.traj_ekin[row * a.n_graphs + g] = (T)s;
    a.traj_epot[row * a.n_graphs + g] = e;
  }
}

template <typename T>
__device__ __forceinline__ void md_join(const MdBackArgs<T>& a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int64_t step_after = a.book[0] + (a.advance ? 1 : 0);
  const int64_t row = md_record_row(a, step_after);
  int bad = 0, wide = 0;
  for (int64_t g = threadIdx.x; g < a.n_graphs; g += blockDim.x) {
    int64_t cb = a.graph_chunk_ptr[g], ce = a.graph_chunk_ptr[g + 1];
    cb = cb < 0 ? 0 : cb;
    ce = ce > a.n_chunks ? a.n_chunks : ce;
    if (ce - cb > MD_JOIN_SERIAL) {
      wide = 1;
      continue;
    }
    double s = 0.0;
    for (int64_t c = cb; c < ce; ++c) {
      s = s + a.partial[c];
      bad |= a.partial_bad[c];
    }
    md_join_store(a, g, row, s, &bad);
  }
  if (__syncthreads_or(wide)) {
    for (int64_t g = wave; g < a.n_graphs; g += waves) {
      int64_t cb = a.graph_chunk_ptr[g], ce = a.graph_chunk_ptr[g + 1];
      cb = cb < 0 ? 0 : cb;
      ce = ce > a.n_chunks ? a.n_chunks : ce;
      if (ce - cb <= MD_JOIN_SERIAL) continue;
      double s = 0.0;
      for (int64_t c = cb + lane; c < ce; c += 64) {
        s = s + a.partial[c];
        bad |= a.partial_bad[c];
      }
      s = md_wave_sum(s);
      if (lane == 0) md_join_store(a, g, row, s, &bad);
    }
  }
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    const int64_t ne = (int64_t)a.n_edges_step[0];
    a.book[0] = step_after;
    if (ne > a.book[1]) a.book[1] = ne;
    if (any_bad) a.book[2] = 1;
    if (row >= 0) a.traj_step[row] = step_after;
  }
}

template <typename T>
__global__ void __launch_bounds__(MD_JOIN_THREADS) k_md_join(MdBackArgs<T> a) {
  md_join(a);
}

// One workgroup per chunk: second half kick, the step's forces into the driver's own copy, the chunk's kinetic energy and non-finite flag.
// (Behind md_join in this file because a lone chunk's workgroup runs it itself.)
template <typename T>
__global__ void __launch_bounds__(MD_CHUNK) k_md_back(MdBackArgs<T> a) {
  __shared__ double wsum[MD_CHUNK / 64];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  int cn = a.chunk_n[c];
  cn = cn < 0 ? 0 : (cn > MD_CHUNK ? MD_CHUNK : cn);
  const int64_t i = (int64_t)a.chunk_atom0[c] + tid;
  double e = 0.0;
  int bad = 0;
  if (tid < cn && i >= 0 && i < a.n) {
    const double im = (double)a.inv_mass[i];
    double v[3];
    for (int k = 0; k < 3; ++k) {
      const T fk = a.frc_step[3 * i + k];
      const double f = (double)fk;
      bad |= !isfinite(f);
      a.frc[3 * i + k] = fk;
      v[k] = (double)a.vel[3 * i + k];
      if (a.advance && im > 0.0) {
        v[k] = (double)(T)(v[k] + a.half_dt * (f * im));
        a.vel[3 * i + k] = (T)v[k];
      }
    }
    e = (double)a.half_mass[i] * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);   // of the STORED velocity: a function of the state alone
    const int64_t row = md_record_row(a, a.book[0] + 1);
    if (row >= 0) {
      for (int j = 0; j < 3; ++j) {
        double x = (double)a.pos[3 * i + j];
        if (a.box.any)
          x = x + (((double)a.image[3 * i] * a.box.cell[j] + (double)a.image[3 * i + 1] * a.box.cell[3 + j]) +
                   (double)a.image[3 * i + 2] * a.box.cell[6 + j]);
        a.traj_pos[(row * a.n + i) * 3 + j] = (T)x;
      }
    }
  }
  e = md_wave_sum(e);
  const int any_bad = __syncthreads_or(bad);
  if ((tid & 63) == 0) wsum[tid >> 6] = e;
  __syncthreads();
  if (tid == 0) {
    double s = wsum[0];
    for (int w = 1; w < MD_CHUNK / 64; ++w) s = s + wsum[w];
    a.partial[c] = s;
    a.partial_bad[c] = any_bad ? 1 : 0;
  }
  if (a.n_chunks == 1) {   // the only chunk (a small molecule, a small box): its workgroup joins and keeps the books itself, one launch less
    __threadfence_block();
    __syncthreads();
    md_join(a);
  }
}

// (host) finite: not NaN and not an infinity
static inline bool md_finite(double x) { return x - x == 0.0; }

static bool md_box(const double* cell, const int32_t* pbc, MdBox* b) {
  b->any = 0;
  for (int k = 0; k < 9; ++k) b->cell[k] = b->inv[k] = 0.0;
  for (int k = 0; k < 3; ++k) b->periodic[k] = (cell && pbc && pbc[k]) ? 1 : 0;
  if (!cell || !(b->periodic[0] || b->periodic[1] || b->periodic[2])) return true;
  const double* c = cell;
  const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
  if (!(det != 0.0) || !md_finite(det)) return false;
  for (int k = 0; k < 9; ++k) b->cell[k] = c[k];
  double* m = b->inv;
  m[0] = (c[4] * c[8] - c[5] * c[7]) / det;
  m[1] = (c[2] * c[7] - c[1] * c[8]) / det;
  m[2] = (c[1] * c[5] - c[2] * c[4]) / det;
  m[3] = (c[5] * c[6] - c[3] * c[8]) / det;
  m[4] = (c[0] * c[8] - c[2] * c[6]) / det;
  m[5] = (c[2] * c[3] - c[0] * c[5]) / det;
  m[6] = (c[3] * c[7] - c[4] * c[6]) / det;
  m[7] = (c[1] * c[6] - c[0] * c[7]) / det;
  m[8] = (c[0] * c[4] - c[1] * c[3]) / det;
  b->any = 1;
  return true;
}

}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_md_inverse_cell(const double* cell, double* inv) {
  XEQ_CHECK_ARG(cell && inv, "xeq_md_inverse_cell: null pointer");
  MdBox b;
  const int32_t all[3] = {1, 1, 1};
  XEQ_CHECK_ARG(md_box(cell, all, &b), "xeq_md_inverse_cell: the cell is singular or not finite");
  for (int k = 0; k < 9; ++k) inv[k] = b.inv[k];
  return XEQ_OK;
}

int xeq_md_normals(int dtype, uint64_t seed, int purpose, uint64_t step, const int64_t* rng_id, int64_t n, uint32_t* words, void* normals,
                   void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_md_normals: dtype %d (0 f32, 1 f64)", dtype);
  XEQ_CHECK_ARG(purpose == XEQ_MD_PURPOSE_LANGEVIN || purpose == XEQ_MD_PURPOSE_MAXWELL, "xeq_md_normals: purpose %d (0 Langevin, 1 Maxwell-Boltzmann)",
                purpose);
  XEQ_CHECK_ARG(step < ((uint64_t)1 << 62), "xeq_md_normals: step %llu does not fit the counter's 62 bits", (unsigned long long)step);
  XEQ_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 31) * 255, "xeq_md_normals: n %lld", (long long)n);
  XEQ_CHECK_ARG(n == 0 || (rng_id && (words || normals)), "xeq_md_normals: null buffer");
  if (n == 0) return XEQ_OK;
  XEQ_DISPATCH_FLOAT(dtype, {
    hipLaunchKernelGGL(k_md_normals<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, purpose, step, rng_id, n, words,
                       (T*)normals);
  });
  XEQ_CHECK_LAUNCH("xeq_md_normals");
  return XEQ_OK;
}

int xeq_md_front(int dtype, int ensemble, int64_t n, int64_t n_graphs, void* pos, void* vel, const void* frc, const void* inv_mass,
                 const int64_t* batch, const void* ke, const void* tfac, const int64_t* rng_id, const int64_t* book, uint64_t seed, double dt,
                 double c1, double noise2, double dt_over_tau, double t0, const double* cell, const int32_t* pbc, int32_t* image, void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_md_front: dtype %d (0 f32, 1 f64)", dtype);
  XEQ_CHECK_ARG(ensemble == XEQ_MD_NVE || ensemble == XEQ_MD_LANGEVIN || ensemble == XEQ_MD_BERENDSEN,
                "xeq_md_front: ensemble %d (0 nve, 1 langevin, 2 berendsen)", ensemble);
  XEQ_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) / 3 && n_graphs >= 0, "xeq_md_front: %lld atoms, %lld graphs", (long long)n, (long long)n_graphs);
  XEQ_CHECK_ARG(md_finite(dt) && dt >= 0.0, "xeq_md_front: time step %g", dt);
  XEQ_CHECK_ARG(ensemble != XEQ_MD_LANGEVIN || (c1 >= 0.0 && c1 <= 1.0 && md_finite(noise2) && noise2 >= 0.0),
                "xeq_md_front: langevin needs 0 <= c1 <= 1 and a finite noise2 >= 0 (got %g, %g)", c1, noise2);
  XEQ_CHECK_ARG(ensemble != XEQ_MD_BERENDSEN || (md_finite(dt_over_tau) && dt_over_tau >= 0.0 && md_finite(t0) && t0 >= 0.0 && n_graphs >= 1),
                "xeq_md_front: berendsen needs dt / tau >= 0, a target temperature >= 0 and a graph (got %g, %g, %lld)", dt_over_tau, t0,
                (long long)n_graphs);
  MdBox box;
  XEQ_CHECK_ARG(md_box(cell, pbc, &box), "xeq_md_front: the cell is singular or not finite");
  XEQ_CHECK_ARG(n == 0 || (pos && vel && frc && inv_mass), "xeq_md_front: null state buffer");
  XEQ_CHECK_ARG(n == 0 || !box.any || image, "xeq_md_front: a periodic system needs the image counts");
  XEQ_CHECK_ARG(n == 0 || ensemble != XEQ_MD_LANGEVIN || (rng_id && book), "xeq_md_front: langevin needs rng_id and the step counter");
  XEQ_CHECK_ARG(n == 0 || ensemble != XEQ_MD_BERENDSEN || (batch && ke && tfac), "xeq_md_front: berendsen needs batch, ke and tfac");
  if (n == 0) return XEQ_OK;
  if (dt == 0.0) ensemble = XEQ_MD_NVE;   // no time passes: no thermostat acts, the wrap alone is left
  XEQ_DISPATCH_FLOAT(dtype, {
    MdFrontArgs<T> a{n, n_graphs, ensemble, (T*)pos, (T*)vel, (const T*)frc, (const T*)inv_mass, batch, (const T*)ke, (const T*)tfac, rng_id, book, seed,
                     dt, c1, noise2, dt_over_tau, t0, image, box};
    hipLaunchKernelGGL(k_md_front<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  });
  XEQ_CHECK_LAUNCH("xeq_md_front");
  return XEQ_OK;
}

int xeq_md_back(int dtype, int advance, int64_t n, int64_t n_graphs, int64_t n_chunks, const void* pos, void* vel, void* frc, const void* frc_step,
                const void* energy_step, const int32_t* n_edges_step, const void* inv_mass, const void* half_mass, const int32_t* chunk_atom0,
                const int32_t* chunk_n, const int32_t* graph_chunk_ptr, double* partial, int32_t* partial_bad, void* ke, void* epot, int64_t* book,
                double half_dt, const double* cell, const int32_t* pbc, const int32_t* image, int64_t record_every, int64_t record_start,
                int64_t record_rows, void* traj_pos, void* traj_epot, void* traj_ekin, int64_t* traj_step, void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_md_back: dtype %d (0 f32, 1 f64)", dtype);
  XEQ_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) / 3 && n_graphs >= 0 && n_chunks >= 0 && n_chunks < ((int64_t)1 << 31),
                "xeq_md_back: %lld atoms, %lld graphs, %lld chunks", (long long)n, (long long)n_graphs, (long long)n_chunks);
  XEQ_CHECK_ARG(n_chunks <= n && n_chunks * XEQ_MD_CHUNK >= n, "xeq_md_back: %lld chunks of at most %d atoms cannot hold %lld atoms", (long long)n_chunks,
                XEQ_MD_CHUNK, (long long)n);
  XEQ_CHECK_ARG(md_finite(half_dt) && half_dt >= 0.0, "xeq_md_back: half time step %g", half_dt);
  XEQ_CHECK_ARG(record_every >= 0 && record_rows >= 0 && record_start >= 0, "xeq_md_back: recorder (%lld, %lld, %lld)", (long long)record_every,
                (long long)record_start, (long long)record_rows);
  MdBox box;
  XEQ_CHECK_ARG(md_box(cell, pbc, &box), "xeq_md_back: the cell is singular or not finite");
  XEQ_CHECK_ARG(book && n_edges_step, "xeq_md_back: null step counter or edge count");
  XEQ_CHECK_ARG(n == 0 || (pos && vel && frc && frc_step && inv_mass && half_mass && chunk_atom0 && chunk_n && partial && partial_bad),
                "xeq_md_back: null per-atom or per-chunk buffer");
  XEQ_CHECK_ARG(n_graphs == 0 || (energy_step && graph_chunk_ptr && ke && epot), "xeq_md_back: null per-graph buffer");
  const bool rec = advance && record_every > 0 && record_rows > 0;
  XEQ_CHECK_ARG(!rec || ((n == 0 || traj_pos) && (n_graphs == 0 || (traj_epot && traj_ekin)) && traj_step), "xeq_md_back: null trajectory buffer");
  XEQ_CHECK_ARG(!rec || n == 0 || !box.any || image, "xeq_md_back: a periodic system's recorder needs the image counts");
  XEQ_DISPATCH_FLOAT(dtype, {
    MdBackArgs<T> a{n, n_graphs, n_chunks, advance ? 1 : 0, (const T*)pos, (T*)vel, (T*)frc, (const T*)frc_step, (const T*)energy_step, n_edges_step,
                    (const T*)inv_mass, (const T*)half_mass, chunk_atom0, chunk_n, graph_chunk_ptr, partial, partial_bad, (T*)ke, (T*)epot, book, half_dt,
                    image, box, rec ? record_every : 0, record_start, record_rows, (T*)traj_pos, (T*)traj_epot, (T*)traj_ekin, traj_step};
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_md_back<T>, dim3((unsigned)n_chunks), dim3(MD_CHUNK), 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_md_back");
    }
    if (n_chunks != 1) hipLaunchKernelGGL(k_md_join<T>, dim3(1), dim3(n_graphs > 64 ? MD_JOIN_THREADS : 256), 0, (hipStream_t)stream, a);
  });
  XEQ_CHECK_LAUNCH("xeq_md_back");
  return XEQ_OK;
}

}  // extern "C"
