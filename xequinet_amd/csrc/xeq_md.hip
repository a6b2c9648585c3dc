// Device-resident molecular dynamics around the whole-step graphs (xequinet_amd/md.py): the integrator's two
// halves -- xeq_md_front in front of the step's graph, xeq_md_back behind it -- and the counter-based generator they share with
// xeq_md_normals; behind them the two halves of the batched FIRE minimiser (xequinet_amd/optimize.py), which share
// the wrap, the chunk sums and the join; the Berendsen barostat's two halves (xeq_npt_front / xeq_npt_back), which
// are the MD halves with a box that lives on the device, the canonical thermostats' two halves (xeq_nvt_front / xeq_nvt_back, DESIGN.md
// section 17), which are the MD halves with a per-graph factor and the thermostat's step in the join, and the kernel that forms the periodic
// search's cell tables from that box (xeq_pbc_tables_device).  Plain vector code, f32 and f64 state.  The box, the wrap, the recorder's rules and the entries' shared argument
// checks are in xeq_resident.h, which xeq_lbfgs.hip includes too.
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
#include "xeq_pbc_tables.h"
#include "xeq_resident.h"

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
  ResBox box;
};

// What a canonical thermostat adds to the front half: nothing (xeq_md_front, xeq_npt_front) ...
struct MdNoFactor {
  template <typename T>
  __device__ __forceinline__ void apply(const MdFrontArgs<T>&, int64_t, double*) const {}
};

// ... or the graph's pending factor (xeq_nvt_front; include/xeq.h: XEQ_NVT_*), which nobody writes in this launch.
struct NvtFactor {
  const double* state;
  bool on;   // dt > 0
  template <typename T>
  __device__ __forceinline__ void apply(const MdFrontArgs<T>& a, int64_t i, double* v) const {
    if (!on) return;
    int64_t g = a.batch[i];
    g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);
    const double s = state[g * XEQ_NVT_ROW + XEQ_NVT_SCALE];
    for (int k = 0; k < 3; ++k) v[k] = s * v[k];
  }
};

// One atom's front half against `box`.  SCALE (the barostat, k_npt_front): x <- mu x for EVERY atom, fixed ones included, between the
// thermostat's scaling and the half kick.  `th`: MdNoFactor or NvtFactor.
template <typename T, bool SCALE, typename Factor>
__device__ __forceinline__ void md_front_atom(const MdFrontArgs<T>& a, int64_t i, const ResBox& box, double mu, const Factor& th) {
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
  th.apply(a, i, v);
  if (SCALE) {
    for (int k = 0; k < 3; ++k) x[k] = mu * x[k];
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
  if (box.any) {
    int32_t img[3] = {a.image[3 * i], a.image[3 * i + 1], a.image[3 * i + 2]};
    res_wrap<T>(box, x, img);
    for (int k = 0; k < 3; ++k) a.image[3 * i + k] = img[k];
  }
  for (int k = 0; k < 3; ++k) {
    a.vel[3 * i + k] = (T)v[k];
    a.pos[3 * i + k] = (T)x[k];
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_md_front(MdFrontArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  md_front_atom<T, false>(a, i, a.box, 1.0, MdNoFactor{});
}

template <typename T>
__global__ void __launch_bounds__(256) k_nvt_front(MdFrontArgs<T> a, NvtFactor th) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  md_front_atom<T, false>(a, i, a.box, 1.0, th);
}

// The barostat's front (xeq_npt_front): the box is the f64 record on the device (include/xeq.h: XEQ_NPT_*).  With dt > 0 every thread
// reads the PENDING cell, its inverse and mu, which nobody writes here; thread 0 alone commits the pending cell to the record's current
// cell and to the step's static cell, which nobody reads here.  dt = 0: the wrap against the current cell, nothing is committed.
template <typename T>
__global__ void __launch_bounds__(256) k_npt_front(MdFrontArgs<T> a, double* rec, T* step_cell) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const bool moves = a.dt > 0.0;
  const double* c = rec + (moves ? XEQ_NPT_CELL_NEXT : XEQ_NPT_CELL);
  const double* m = rec + (moves ? XEQ_NPT_INV_NEXT : XEQ_NPT_INV);
  ResBox box;
  for (int k = 0; k < 9; ++k) {
    box.cell[k] = c[k];
    box.inv[k] = m[k];
  }
  box.periodic[0] = box.periodic[1] = box.periodic[2] = box.any = 1;
  const double mu = moves ? rec[XEQ_NPT_MU] : 1.0;
  md_front_atom<T, true>(a, i, box, mu, MdNoFactor{});
  if (i == 0 && moves) {
    for (int k = 0; k < 9; ++k) {
      rec[XEQ_NPT_CELL + k] = box.cell[k];
      rec[XEQ_NPT_INV + k] = box.inv[k];
      step_cell[k] = (T)box.cell[k];
    }
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
  ResBox box;
  int64_t record_every, record_start, record_rows;
  T* traj_pos;
  T* traj_epot;
  T* traj_ekin;
  int64_t* traj_step;
};

// The MD backs record with `advance` alone.
template <typename T>
__device__ __forceinline__ int64_t md_record_row(const MdBackArgs<T>& a, int64_t step_after) {
  return a.advance ? res_record_row(a.record_every, a.record_start, a.record_rows, step_after) : -1;
}

// One workgroup joins every graph's chunk partials in chunk order.  A graph of at most MD_JOIN_SERIAL chunks is summed by one lane, chunk
// after chunk (a batch of many small molecules: a graph per lane); a larger one by a wave, lane l adding chunks l, l + 64, ... and a
// butterfly.  Which of the two depends on the graph's own chunk count alone.  `make()` gives an empty accumulator with add(chunk) and
// wave() (the butterfly); `done(g, acc)` is called by the one lane that holds the graph's sum.  (The MD and the FIRE joins share this.)
template <typename Make, typename Done>
__device__ __forceinline__ void md_join_graphs(int64_t n_graphs, int64_t n_chunks, const int32_t* __restrict__ graph_chunk_ptr, Make make, Done done) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int wide = 0;
  for (int64_t g = threadIdx.x; g < n_graphs; g += blockDim.x) {
    int64_t cb = graph_chunk_ptr[g], ce = graph_chunk_ptr[g + 1];
    cb = cb < 0 ? 0 : cb;
    ce = ce > n_chunks ? n_chunks : ce;
    if (ce - cb > MD_JOIN_SERIAL) {
      wide = 1;
      continue;
    }
    auto s = make();
    for (int64_t c = cb; c < ce; ++c) s.add(c);
    done(g, s);
  }
  if (__syncthreads_or(wide)) {
    for (int64_t g = wave; g < n_graphs; g += waves) {
      int64_t cb = graph_chunk_ptr[g], ce = graph_chunk_ptr[g + 1];
      cb = cb < 0 ? 0 : cb;
      ce = ce > n_chunks ? n_chunks : ce;
      if (ce - cb <= MD_JOIN_SERIAL) continue;
      auto s = make();
      for (int64_t c = cb + lane; c < ce; c += 64) s.add(c);
      s.wave();
      if (lane == 0) done(g, s);
    }
  }
}

struct MdKeSum {
  const double* partial;
  const int32_t* partial_bad;
  double s;
  int bad;
  __device__ __forceinline__ void add(int64_t c) {
    s = s + partial[c];
    bad |= partial_bad[c];
  }
  __device__ __forceinline__ void wave() {
    s = res_wave_sum(s);
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);   // (the one lane that stores carries every lane's flag)
  }
};

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

// What a canonical thermostat adds to the join: nothing, the graph's kinetic energy is its sum (xeq_md_back, xeq_npt_back) ...
struct MdNoThermostat {
  template <typename T>
  __device__ __forceinline__ double kinetic(const MdBackArgs<T>&, int64_t, int64_t, double k, int*) const {
    return k;
  }
};

// ... or one thermostat step of the graph (xeq_nvt_back), run by the lane that holds the graph's sum K behind step number `step`: the
// statement of include/xeq.h (XEQ_NVT_*), operation by operation; tests/nvt_oracle.py restates it in numpy.  O(1) whatever the graph's size.
struct NvtThermostat {
  int kind, chain;
  double* state;
  const int64_t* n_free;
  const int64_t* graph_rng_id;
  uint64_t seed;
  double kT, tau, dt;

  // One pass of the chain's velocity updates: k = M .. 1 (`down`) or 1 .. M.  Fully unrolled: vxi stays in registers.
  __device__ __forceinline__ void chain_velocities(double* vxi, double k_now, double nfkT, double q1, double q, double hd, double qd, bool down) const {
#pragma unroll
    for (int j = 0; j < XEQ_NVT_MAX_CHAIN; ++j) {
      const int k = down ? XEQ_NVT_MAX_CHAIN - 1 - j : j;   // (0-based)
      if (k >= chain) continue;
      double gk;
      if (k == 0) {
        gk = (2.0 * k_now - nfkT) / q1;
      } else {
        const double qp = k == 1 ? q1 : q;
        gk = (qp * (vxi[k - 1] * vxi[k - 1]) - kT) / q;
      }
      if (k == chain - 1) {
        vxi[k] = vxi[k] + hd * gk;
      } else {
        const double e = exp(-(qd * vxi[k + 1 < XEQ_NVT_MAX_CHAIN ? k + 1 : k]));
        vxi[k] = vxi[k] * e;
        vxi[k] = vxi[k] + hd * gk;
        vxi[k] = vxi[k] * e;
      }
    }
  }

  __device__ __forceinline__ double nose_hoover(double* row, double k_now, double nf) const {
    double xi[XEQ_NVT_MAX_CHAIN], vxi[XEQ_NVT_MAX_CHAIN];
#pragma unroll
    for (int k = 0; k < XEQ_NVT_MAX_CHAIN; ++k) {
      xi[k] = row[XEQ_NVT_XI + k];
      vxi[k] = row[XEQ_NVT_VXI + k];
    }
    const double nfkT = nf * kT, tau2 = tau * tau;
    const double q1 = nfkT * tau2, q = kT * tau2;
    const double delta = dt / 2.0, hd = 0.5 * delta, qd = 0.25 * delta;
    double s = 1.0;
    for (int half = 0; half < 2; ++half) {
      chain_velocities(vxi, k_now, nfkT, q1, q, hd, qd, true);
      const double sigma = exp(-(delta * vxi[0]));
      k_now = (sigma * sigma) * k_now;
      s = s * sigma;
#pragma unroll
      for (int k = 0; k < XEQ_NVT_MAX_CHAIN; ++k) {
        if (k < chain) xi[k] = xi[k] + delta * vxi[k];
      }
      chain_velocities(vxi, k_now, nfkT, q1, q, hd, qd, false);
    }
    if (!(isfinite(s) && s > 0.0)) return s;
    double b = 0.0, t = 0.0;
#pragma unroll
    for (int k = 0; k < XEQ_NVT_MAX_CHAIN; ++k) {
      if (k < chain) b = b + 0.5 * ((k == 0 ? q1 : q) * (vxi[k] * vxi[k]));
    }
    b = b + nfkT * xi[0];
#pragma unroll
    for (int k = 1; k < XEQ_NVT_MAX_CHAIN; ++k) {
      if (k < chain) t = t + xi[k];
    }
    b = b + kT * t;
    row[XEQ_NVT_BATH] = b;
#pragma unroll
    for (int k = 0; k < XEQ_NVT_MAX_CHAIN; ++k) {
      if (k < chain) {
        row[XEQ_NVT_XI + k] = xi[k];
        row[XEQ_NVT_VXI + k] = vxi[k];
      }
    }
    return s;
  }

  // z0, z1 in double and u = (word_2 + 1) 2^-32 of block j of (graph, step).
  __device__ __forceinline__ void draw(int64_t id, int j, int64_t step, double z[3], double* u) const {
    uint32_t w[4];
    md_block(seed, XEQ_NVT_PURPOSE, id | (int64_t)j, (uint64_t)step, w);
    md_normals3<double>(w, z);
    *u = ((double)w[2] + 1.0) * 2.3283064365386962890625e-10;
  }

  __device__ __forceinline__ double bussi(double* row, int64_t g, int64_t step, double k_now, int64_t nf_int) const {
    const double nf = (double)nf_int;
    const int64_t id = graph_rng_id[g];
    double z[3], u;
    draw(id, 0, step, z, &u);
    const double r = z[0];
    const bool even = ((nf_int - 1) & 1) == 0;
    const double a = (double)((even ? nf_int - 1 : nf_int - 2) / 2);
    const double d = a - 1.0 / 3.0, cp = 1.0 / sqrt(9.0 * d);
    double gam = 0.0;
    for (int j = 1; j <= XEQ_NVT_GAMMA_TRIES; ++j) {
      double zj[3];
      draw(id, j, step, zj, &u);
      const double x = zj[0], t = 1.0 + cp * x, v = (t * t) * t;
      gam = d * fabs(v);
      if (v > 0.0 && log(u) < ((0.5 * (x * x) + d) - d * v) + d * log(v)) break;
    }
    const double sdraw = even ? 2.0 * gam : 2.0 * gam + z[1] * z[1];
    const double c = exp(-(dt / tau));
    const double q = ((1.0 - c) * (0.5 * (nf * kT))) / (nf * k_now);
    const double s2 = (c + q * (r * r + sdraw)) + (2.0 * r) * sqrt(c * q);
    const double s = sqrt(s2);
    if (isfinite(s) && s > 0.0) row[XEQ_NVT_BATH] = row[XEQ_NVT_BATH] - (s2 - 1.0) * k_now;
    return s;
  }

  template <typename T>
  __device__ __forceinline__ double kinetic(const MdBackArgs<T>& a, int64_t g, int64_t step, double k_sum, int* bad) const {
    double* row = state + g * XEQ_NVT_ROW;
    double s = 1.0;
    const int64_t nf = 3 * n_free[g];
    if (a.advance && nf > 0 && k_sum > 0.0) {
      s = kind == XEQ_NVT_BUSSI ? bussi(row, g, step, k_sum, nf) : nose_hoover(row, k_sum, (double)nf);
      if (!(isfinite(s) && s > 0.0)) {
        *bad |= !isfinite(s);
        s = 1.0;
      }
    }
    row[XEQ_NVT_SCALE] = s;
    return (s * s) * k_sum;
  }
};

// What the NVT ensembles add to the back half: nothing; the recorder's cell is the launch's own.
struct MdNoBox {
  template <typename T>
  __device__ __forceinline__ const double* cell(const MdBackArgs<T>& a) const {
    return a.box.cell;
  }
  template <typename T>
  __device__ __forceinline__ void finish(const MdBackArgs<T>&, int64_t) const {}
};

// The Berendsen barostat (xeq_npt_back), run by the ONE lane that keeps the books, behind them: the pressure of the state this launch
// leaves, the scale factor of the NEXT step and the cell it will have, into the f64 record.  All in double, in the order written.
template <typename T>
struct NptBox {
  const T* virial_step;
  T* virial;
  double* rec;
  const int32_t* reps_needed;
  int32_t* reps_seen;
  int32_t reps[3];
  double kappa, p0, p_unit;
  T* traj_cell;
  double* traj_pressure;
  __device__ __forceinline__ const double* cell(const MdBackArgs<T>&) const { return rec + XEQ_NPT_CELL; }
  __device__ __forceinline__ void finish(const MdBackArgs<T>& a, int64_t row) const {
    const double* c = rec + XEQ_NPT_CELL;
    double w[9];
    for (int k = 0; k < 9; ++k) {
      const T wk = virial_step[k];
      virial[k] = wk;
      w[k] = (double)wk;
    }
    const double vol = fabs(md_det(c));
    const double p = (2.0 * (double)a.ke[0] + ((w[0] + w[4]) + w[8])) / (3.0 * vol);
    double mu = 1.0 - kappa * (p0 - p);
    int bad = 0;
    if (!(mu > 0.0) || !isfinite(mu)) {
      bad = 1;
      mu = 1.0;
    }
    double cn[9], in[9];
    for (int k = 0; k < 9; ++k) cn[k] = (double)(T)(mu * c[k]);
    const double dn = md_inverse(cn, in);
    if (!(dn != 0.0) || !isfinite(dn)) {   // (a box the next step could not wrap against: it stays, the window is void)
      bad = 1;
      mu = 1.0;
      for (int k = 0; k < 9; ++k) {
        cn[k] = c[k];
        in[k] = rec[XEQ_NPT_INV + k];
      }
    }
    for (int k = 0; k < 9; ++k) {
      rec[XEQ_NPT_CELL_NEXT + k] = cn[k];
      rec[XEQ_NPT_INV_NEXT + k] = in[k];
    }
    rec[XEQ_NPT_MU] = mu;
    rec[XEQ_NPT_P] = p;
    rec[XEQ_NPT_V] = vol;
    if (bad) a.book[2] = 1;
    if (reps_needed) {
      for (int k = 0; k < 3; ++k) {
        const int32_t r = reps_needed[k];
        if (r > reps[k]) a.book[3] = 1;
        if (r > reps_seen[k]) reps_seen[k] = r;
      }
    }
    if (row >= 0) {
      for (int k = 0; k < 9; ++k) traj_cell[9 * row + k] = (T)c[k];
      traj_pressure[row] = p * p_unit;
    }
  }
};

// The MD join; then ONE lane does the bookkeeping with plain stores.  `th`: MdNoThermostat or NvtThermostat.
template <typename T, typename Box, typename Thermostat>
__device__ __forceinline__ void md_join(const MdBackArgs<T>& a, const Box& bx, const Thermostat& th) {
  const int64_t step_after = a.book[0] + (a.advance ? 1 : 0);
  const int64_t row = md_record_row(a, step_after);
  int bad = 0;
  md_join_graphs(
      a.n_graphs, a.n_chunks, a.graph_chunk_ptr, [&]() { return MdKeSum{a.partial, a.partial_bad, 0.0, 0}; },
      [&](int64_t g, const MdKeSum& k) {
        bad |= k.bad;
        md_join_store(a, g, row, th.kinetic(a, g, step_after - (a.advance ? 1 : 0), k.s, &bad), &bad);
      });
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    const int64_t ne = (int64_t)a.n_edges_step[0];
    a.book[0] = step_after;
    if (ne > a.book[1]) a.book[1] = ne;
    if (any_bad) a.book[2] = 1;
    if (row >= 0) a.traj_step[row] = step_after;
    bx.finish(a, row);
  }
}

template <typename T>
__global__ void __launch_bounds__(MD_JOIN_THREADS) k_md_join(MdBackArgs<T> a) {
  md_join(a, MdNoBox{}, MdNoThermostat{});
}

template <typename T>
__global__ void __launch_bounds__(MD_JOIN_THREADS) k_nvt_join(MdBackArgs<T> a, NvtThermostat th) {
  md_join(a, MdNoBox{}, th);
}

template <typename T>
__global__ void __launch_bounds__(MD_JOIN_THREADS) k_npt_join(MdBackArgs<T> a, NptBox<T> bx) {
  md_join(a, bx, MdNoThermostat{});
}

// One workgroup per chunk: second half kick, the step's forces into the driver's own copy, the chunk's kinetic energy and non-finite flag.
// (Behind md_join in this file because a lone chunk's workgroup runs it itself.)
template <typename T, typename Box, typename Thermostat>
__device__ __forceinline__ void md_back_chunk(const MdBackArgs<T>& a, const Box& bx, const Thermostat& th) {
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
    if (row >= 0) res_store_unwrapped(a.traj_pos, row, a.n, i, a.pos, a.image, a.box.any, bx.cell(a));
  }
  e = res_wave_sum(e);
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
    md_join(a, bx, th);
  }
}

template <typename T>
__global__ void __launch_bounds__(MD_CHUNK) k_md_back(MdBackArgs<T> a) {
  md_back_chunk(a, MdNoBox{}, MdNoThermostat{});
}

template <typename T>
__global__ void __launch_bounds__(MD_CHUNK) k_nvt_back(MdBackArgs<T> a, NvtThermostat th) {
  md_back_chunk(a, MdNoBox{}, th);
}

template <typename T>
__global__ void __launch_bounds__(MD_CHUNK) k_npt_back(MdBackArgs<T> a, NptBox<T> bx) {
  md_back_chunk(a, bx, MdNoThermostat{});
}

// ------------------------------------------------------------------------------------------------------------- cell tables
// xeq_pbc_tables_device: the flat table grid | offs | recip | thr of ONE cell that lives on the device, by the statement the host
// function uses (xeq_pbc_tables.h); this file is built without contraction.  Thread k forms image k; thread 0 also the cell's geometry.
struct Reps3 {
  int32_t reps[3], pbc[3];
};

template <typename T>
__global__ void __launch_bounds__(256) k_pbc_tables(const T* __restrict__ cell, Reps3 r, int64_t nc, double cutoff, T* __restrict__ out,
                                                    int32_t* __restrict__ reps_needed) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nc) return;
  T a[9];
  for (int j = 0; j < 9; ++j) a[j] = cell[j];
  T grid[3], offs[3];
  cell_table_image<T>(a, r.reps, k, grid, offs);
  for (int j = 0; j < 3; ++j) {
    out[3 * k + j] = grid[j];
    out[3 * (nc + k) + j] = offs[j];
  }
  if (k == 0) {
    CellGeom<T> cg;
    cell_geom<T>(a, cg);
    T recip[9], thr[3];
    cell_table_prune<T>(cg, cutoff, recip, thr);
    for (int j = 0; j < 9; ++j) out[6 * nc + j] = recip[j];
    for (int j = 0; j < 3; ++j) out[6 * nc + 9 + j] = thr[j];
    if (reps_needed) {
      for (int ax = 0; ax < 3; ++ax) reps_needed[ax] = r.pbc[ax] ? cell_image_count<T>(cg, ax, cutoff) : 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- FIRE
// Batched geometry optimisation around the same whole-step graphs (xequinet_amd/optimize.py): every graph is its
// own FIRE system (Bitzek et al., PRL 97, 170201 (2006), in the form of ASE's optimize.FIRE).  xeq_fire_back behind an evaluation forms a
// graph's P = sum f.v, ff = sum f.f, vv = sum v.v and max |f_i|^2 over its free atoms -- chunk partials and join exactly as the kinetic
// energy above -- and the lane that holds them runs the graph's state machine; xeq_fire_front in front of the next evaluation moves the
// atoms by the three coefficients that lane left.  The per-graph state (dt, alpha, c_v, c_f, d) is double whatever the state's type.
template <typename T>
struct FireBackArgs {
  int64_t n, n_graphs, n_chunks;
  const T* pos;
  const T* vel;
  T* frc;
  const T* frc_step;
  const T* energy_step;
  const int32_t* n_edges_step;
  const uint8_t* fixed;
  const int64_t* batch;
  const int32_t* chunk_atom0;
  const int32_t* chunk_n;
  const int32_t* graph_chunk_ptr;
  double* partial;   // [n_chunks, 4]: P, ff, vv, max |f|^2
  int32_t* partial_bad;
  T* epot;
  T* fmax;
  double* dt;
  double* alpha;
  int32_t* n_pos;
  int32_t* status;
  int64_t* converged_at;
  double* coef;   // [n_graphs, 3]: c_v, c_f, d
  int64_t* book;
  double fmax_tol, maxstep, dtmax, f_inc, f_dec, alpha_start, f_alpha;
  int n_min;
  const int32_t* image;
  ResBox box;
  int64_t record_every, record_start, record_rows;
  T* traj_pos;
  T* traj_epot;
  T* traj_fmax;
  int64_t* traj_step;
};

struct FireSums {
  const double* partial;
  const int32_t* partial_bad;
  double p, ff, vv, m2;
  int bad;
  __device__ __forceinline__ void add(int64_t c) {
    p = p + partial[4 * c];
    ff = ff + partial[4 * c + 1];
    vv = vv + partial[4 * c + 2];
    m2 = fmax(m2, partial[4 * c + 3]);
    bad |= partial_bad[c];
  }
  __device__ __forceinline__ void wave() {
    p = res_wave_sum(p);
    ff = res_wave_sum(ff);
    vv = res_wave_sum(vv);
    m2 = res_wave_max(m2);
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  }
};

// One graph's state machine, run by the lane that holds its sums behind evaluation number `eval`.  A converged graph is left alone, bit
// for bit; only its recorder row is filled, from what it kept.
template <typename T>
__device__ __forceinline__ void fire_decide(const FireBackArgs<T>& a, int64_t g, int64_t row, int64_t eval, const FireSums& s, int* bad) {
  const int st = a.status[g];
  if (st != XEQ_FIRE_CONVERGED) {
    const T e = a.energy_step[g];
    *bad |= s.bad | !isfinite((double)e);
    const double fm = sqrt(s.m2);
    a.epot[g] = e;
    a.fmax[g] = (T)fm;
    if (fm < a.fmax_tol) {
      a.status[g] = XEQ_FIRE_CONVERGED;
      a.converged_at[g] = eval;
    } else {
      double dt = a.dt[g], al = a.alpha[g], cv, cf;
      int np = a.n_pos[g];
      if (st == XEQ_FIRE_FRESH) {
        cv = 0.0;
        cf = dt;
      } else if (s.p > 0.0) {
        const double al_old = al;
        cv = 1.0 - al;
        if (np > a.n_min) {
          dt = fmin(dt * a.f_inc, a.dtmax);
          al = al * a.f_alpha;
        }
        np = np + 1;
        cf = al_old * sqrt(s.vv) / sqrt(s.ff) + dt;
      } else {
        cv = 0.0;
        al = a.alpha_start;
        dt = dt * a.f_dec;
        np = 0;
        cf = dt;
      }
      const double vn2 = ((cv * cv) * s.vv + ((2.0 * cv) * cf) * s.p) + (cf * cf) * s.ff;   // |c_v v + c_f f|^2 from the same three sums
      const double norm = dt * sqrt(fmax(vn2, 0.0));
      const double d = norm > a.maxstep ? dt * (a.maxstep / norm) : dt;
      a.dt[g] = dt;
      a.alpha[g] = al;
      a.n_pos[g] = np;
      a.status[g] = XEQ_FIRE_ACTIVE;
      a.coef[3 * g] = cv;
      a.coef[3 * g + 1] = cf;
      a.coef[3 * g + 2] = d;
    }
  }
  if (row >= 0) {
    a.traj_epot[row * a.n_graphs + g] = a.epot[g];
    a.traj_fmax[row * a.n_graphs + g] = a.fmax[g];
  }
}

template <typename T>
__device__ __forceinline__ void fire_join(const FireBackArgs<T>& a) {
  const int64_t eval = a.book[0];   // this evaluation's number: the first one is 0
  const int64_t row = res_record_row(a.record_every, a.record_start, a.record_rows, eval);
  int bad = 0;
  md_join_graphs(
      a.n_graphs, a.n_chunks, a.graph_chunk_ptr, [&]() { return FireSums{a.partial, a.partial_bad, 0.0, 0.0, 0.0, 0.0, 0}; },
      [&](int64_t g, const FireSums& s) { fire_decide(a, g, row, eval, s, &bad); });
  const int any_bad = __syncthreads_or(bad);   // (also orders the status stores above before the count below)
  int64_t active = 0;
  for (int64_t base = 0; base < a.n_graphs; base += blockDim.x) {
    const int64_t g = base + threadIdx.x;
    active += __syncthreads_count(g < a.n_graphs && a.status[g] != XEQ_FIRE_CONVERGED);
  }
  if (threadIdx.x == 0) {
    const int64_t ne = (int64_t)a.n_edges_step[0];
    a.book[0] = eval + 1;
    if (ne > a.book[1]) a.book[1] = ne;
    if (any_bad) a.book[2] = 1;
    a.book[3] = active;
    if (row >= 0) a.traj_step[row] = eval;
  }
}

template <typename T>
__global__ void __launch_bounds__(MD_JOIN_THREADS) k_fire_join(FireBackArgs<T> a) {
  fire_join(a);
}

// One workgroup per chunk: the step's forces into the driver's copy (a fixed atom's entry zero, a converged graph's left alone), the
// chunk's four partials over its free atoms and its non-finite flag, the recorder's positions.
template <typename T>
__global__ void __launch_bounds__(MD_CHUNK) k_fire_back(FireBackArgs<T> a) {
  __shared__ double wsum[4][MD_CHUNK / 64];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  int cn = a.chunk_n[c];
  cn = cn < 0 ? 0 : (cn > MD_CHUNK ? MD_CHUNK : cn);
  const int64_t i = (int64_t)a.chunk_atom0[c] + tid;
  double p = 0.0, ff = 0.0, vv = 0.0;
  int bad = 0;
  if (tid < cn && i >= 0 && i < a.n) {
    int64_t g = a.batch[i];
    g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);
    const bool frozen = a.status[g] == XEQ_FIRE_CONVERGED;
    const bool fix = a.fixed && a.fixed[i];
    double f[3], v[3];
    for (int k = 0; k < 3; ++k) {
      const T fk = a.frc_step[3 * i + k];
      bad |= !isfinite((double)fk);
      f[k] = fix ? 0.0 : (double)fk;
      v[k] = fix ? 0.0 : (double)a.vel[3 * i + k];
      if (!frozen) a.frc[3 * i + k] = fix ? T(0) : fk;
    }
    p = (f[0] * v[0] + f[1] * v[1]) + f[2] * v[2];
    ff = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
    vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const int64_t row = res_record_row(a.record_every, a.record_start, a.record_rows, a.book[0]);
    if (row >= 0) {   // res_store_unwrapped, written out: through the helper this kernel takes 8 more SGPRs (profiles/resident_shared_refactor.txt)
      for (int j = 0; j < 3; ++j) {
        double x = (double)a.pos[3 * i + j];
        if (a.box.any)
          x = x + (((double)a.image[3 * i] * a.box.cell[j] + (double)a.image[3 * i + 1] * a.box.cell[3 + j]) +
                   (double)a.image[3 * i + 2] * a.box.cell[6 + j]);
        a.traj_pos[(row * a.n + i) * 3 + j] = (T)x;
      }
    }
  }
  const double m2 = res_wave_max(ff);   // (a lane's ff IS its atom's |f|^2)
  p = res_wave_sum(p);
  ff = res_wave_sum(ff);
  vv = res_wave_sum(vv);
  const int any_bad = __syncthreads_or(bad);
  if ((tid & 63) == 0) {
    wsum[0][tid >> 6] = p;
    wsum[1][tid >> 6] = ff;
    wsum[2][tid >> 6] = vv;
    wsum[3][tid >> 6] = m2;
  }
  __syncthreads();
  if (tid < 4) {
    double s = wsum[tid][0];
    for (int w = 1; w < MD_CHUNK / 64; ++w) s = tid == 3 ? fmax(s, wsum[tid][w]) : s + wsum[tid][w];
    a.partial[4 * (int64_t)c + tid] = s;
    if (tid == 0) a.partial_bad[c] = any_bad ? 1 : 0;
  }
  if (a.n_chunks == 1) {   // the only chunk: its workgroup joins, decides and keeps the books itself, one launch less
    __threadfence_block();
    __syncthreads();
    fire_join(a);
  }
}

template <typename T>
struct FireFrontArgs {
  int64_t n, n_graphs;
  T* pos;
  T* vel;
  const T* frc;
  const uint8_t* fixed;
  const int64_t* batch;
  const int32_t* status;
  const double* coef;
  int32_t* image;
  ResBox box;
};

// Per free atom of a graph that is not converged: v = c_v v + c_f f, x += d v, the wrap.  Nothing else is written.
template <typename T>
__global__ void __launch_bounds__(256) k_fire_front(FireFrontArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.fixed && a.fixed[i]) return;
  int64_t g = a.batch[i];
  g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);
  if (a.status[g] != XEQ_FIRE_ACTIVE) return;   // converged, or never evaluated: there are no coefficients
  const double cv = a.coef[3 * g], cf = a.coef[3 * g + 1], d = a.coef[3 * g + 2];
  double v[3], x[3];
  for (int k = 0; k < 3; ++k) {
    v[k] = cv * (double)a.vel[3 * i + k] + cf * (double)a.frc[3 * i + k];
    x[k] = (double)a.pos[3 * i + k] + d * v[k];
  }
  if (a.box.any) {
    int32_t img[3] = {a.image[3 * i], a.image[3 * i + 1], a.image[3 * i + 2]};
    res_wrap<T>(a.box, x, img);
    for (int k = 0; k < 3; ++k) a.image[3 * i + k] = img[k];
  }
  for (int k = 0; k < 3; ++k) {
    a.vel[3 * i + k] = (T)v[k];
    a.pos[3 * i + k] = (T)x[k];
  }
}

// The kernel arguments of xeq_md_back and xeq_npt_back from the records; `on`: the recorder records in this call.
template <typename T>
static MdBackArgs<T> md_back_args(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                                  const xeq_res_recorder* rec, int64_t n_graphs, int advance, const ResBox& box, bool on) {
  return MdBackArgs<T>{sys->n, n_graphs, sys->n_chunks, advance ? 1 : 0, (const T*)sys->pos, (T*)sys->vel, (T*)sys->frc, (const T*)step->frc_step,
                       (const T*)step->energy_step, step->n_edges_step, (const T*)md->inv_mass, (const T*)md->half_mass, chunks->chunk_atom0,
                       chunks->chunk_n, chunks->graph_chunk_ptr, chunks->partial, chunks->partial_bad, (T*)md->ke, (T*)md->epot, sys->book, md->half_dt,
                       sys->image, box, on ? rec->every : 0, rec->start, rec->rows, (T*)rec->traj_pos, (T*)rec->traj_epot, (T*)rec->traj_second,
                       rec->traj_step};
}

}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_md_inverse_cell(const double* cell, double* inv) {
  XEQ_CHECK_ARG(cell && inv, "xeq_md_inverse_cell: null pointer");
  ResBox b;
  const int32_t all[3] = {1, 1, 1};
  XEQ_CHECK_ARG(res_box_of(cell, all, &b), "xeq_md_inverse_cell: the cell is singular or not finite");
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

int64_t xeq_record_bytes(int which) {
  switch (which) {
    case XEQ_REC_SYSTEM: return sizeof(xeq_res_system);
    case XEQ_REC_STEP: return sizeof(xeq_res_step);
    case XEQ_REC_CHUNKS: return sizeof(xeq_res_chunks);
    case XEQ_REC_RECORDER: return sizeof(xeq_res_recorder);
    case XEQ_REC_MD: return sizeof(xeq_md_params);
    case XEQ_REC_NPT: return sizeof(xeq_npt_params);
    case XEQ_REC_FIRE: return sizeof(xeq_fire_params);
    case XEQ_REC_NEIGHBORS: return sizeof(xeq_neighbor_search);
    case XEQ_REC_LBFGS: return sizeof(xeq_lbfgs_params);
    case XEQ_REC_NVT: return sizeof(xeq_nvt_params);
  }
  return -1;
}

int xeq_md_front(const xeq_res_system* sys, const xeq_md_params* md, double dt, void* stream) {
  const char* who = "xeq_md_front";
  RES_TRY(res_dtype(who, sys, md));
  XEQ_CHECK_ARG(md->ensemble == XEQ_MD_NVE || md->ensemble == XEQ_MD_LANGEVIN || md->ensemble == XEQ_MD_BERENDSEN,
                "xeq_md_front: ensemble %lld (0 nve, 1 langevin, 2 berendsen)", (long long)md->ensemble);
  int ensemble = (int)md->ensemble;
  const int64_t n = sys->n, n_graphs = sys->n_graphs;
  RES_TRY(res_atoms_graphs(who, sys));
  XEQ_CHECK_ARG(res_finite(dt) && dt >= 0.0, "xeq_md_front: time step %g", dt);
  XEQ_CHECK_ARG(ensemble != XEQ_MD_LANGEVIN || (md->c1 >= 0.0 && md->c1 <= 1.0 && res_finite(md->noise2) && md->noise2 >= 0.0),
                "xeq_md_front: langevin needs 0 <= c1 <= 1 and a finite noise2 >= 0 (got %g, %g)", md->c1, md->noise2);
  XEQ_CHECK_ARG(ensemble != XEQ_MD_BERENDSEN ||
                    (res_finite(md->dt_over_tau) && md->dt_over_tau >= 0.0 && res_finite(md->t0) && md->t0 >= 0.0 && n_graphs >= 1),
                "xeq_md_front: berendsen needs dt / tau >= 0, a target temperature >= 0 and a graph (got %g, %g, %lld)", md->dt_over_tau, md->t0,
                (long long)n_graphs);
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(n == 0 || (sys->pos && sys->vel && sys->frc && md->inv_mass), "xeq_md_front: null state buffer");
  XEQ_CHECK_ARG(n == 0 || !box.any || sys->image, "xeq_md_front: a periodic system needs the image counts");
  XEQ_CHECK_ARG(n == 0 || ensemble != XEQ_MD_LANGEVIN || (md->rng_id && sys->book), "xeq_md_front: langevin needs rng_id and the step counter");
  XEQ_CHECK_ARG(n == 0 || ensemble != XEQ_MD_BERENDSEN || (sys->batch && md->ke && md->tfac), "xeq_md_front: berendsen needs batch, ke and tfac");
  if (n == 0) return XEQ_OK;
  if (dt == 0.0) ensemble = XEQ_MD_NVE;   // no time passes: no thermostat acts, the wrap alone is left
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    MdFrontArgs<T> a{n, n_graphs, ensemble, (T*)sys->pos, (T*)sys->vel, (const T*)sys->frc, (const T*)md->inv_mass, sys->batch, (const T*)md->ke,
                     (const T*)md->tfac, md->rng_id, sys->book, md->seed, dt, md->c1, md->noise2, md->dt_over_tau, md->t0, sys->image, box};
    hipLaunchKernelGGL(k_md_front<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  });
  XEQ_CHECK_LAUNCH("xeq_md_front");
  return XEQ_OK;
}

int xeq_md_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                const xeq_res_recorder* rec, int advance, void* stream) {
  const char* who = "xeq_md_back";
  RES_TRY(res_dtype(who, sys, step && chunks && md));
  if (!rec) rec = &RES_NO_RECORDER;
  const int64_t n = sys->n, n_graphs = sys->n_graphs, n_chunks = sys->n_chunks;
  RES_TRY(res_back_sizes(who, sys, (int64_t)1 << 31));
  XEQ_CHECK_ARG(res_finite(md->half_dt) && md->half_dt >= 0.0, "xeq_md_back: half time step %g", md->half_dt);
  RES_TRY(res_recorder(who, rec));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(sys->book && step->n_edges_step, "xeq_md_back: null step counter or edge count");
  XEQ_CHECK_ARG(n == 0 || (res_back_buffers(sys, step, chunks, true) && md->inv_mass && md->half_mass), "xeq_md_back: null per-atom or per-chunk buffer");
  XEQ_CHECK_ARG(n_graphs == 0 || (step->energy_step && chunks->graph_chunk_ptr && md->ke && md->epot), "xeq_md_back: null per-graph buffer");
  const bool on = advance && rec->every > 0 && rec->rows > 0;
  if (on) RES_TRY(res_trajectory(who, sys, rec, box));
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    const MdBackArgs<T> a = md_back_args<T>(sys, step, chunks, md, rec, n_graphs, advance, box, on);
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_md_back<T>, dim3((unsigned)n_chunks), dim3(MD_CHUNK), 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_md_back");
    }
    if (n_chunks != 1) hipLaunchKernelGGL(k_md_join<T>, dim3(1), dim3(n_graphs > 64 ? MD_JOIN_THREADS : 256), 0, (hipStream_t)stream, a);
  });
  XEQ_CHECK_LAUNCH("xeq_md_back");
  return XEQ_OK;
}

int xeq_pbc_tables_device(int dtype, const void* cell, const int32_t reps[3], const int32_t pbc[3], double cutoff, void* out, int64_t out_count,
                          int32_t* reps_needed, void* stream) {
  XEQ_CHECK_ARG(dtype == XEQ_F32 || dtype == XEQ_F64, "xeq_pbc_tables_device: dtype %d (0 f32, 1 f64)", dtype);
  XEQ_CHECK_ARG(cell && out && reps && pbc, "xeq_pbc_tables_device: null pointer");
  XEQ_CHECK_ARG(res_finite(cutoff) && cutoff > 0.0, "xeq_pbc_tables_device: cutoff %g", cutoff);
  XEQ_CHECK_ARG(reps[0] >= 0 && reps[1] >= 0 && reps[2] >= 0 && reps[0] <= 64 && reps[1] <= 64 && reps[2] <= 64,
                "xeq_pbc_tables_device: %d x %d x %d images per axis (0 .. 64 each)", reps[0], reps[1], reps[2]);
  const int64_t nc = (int64_t)(2 * reps[0] + 1) * (2 * reps[1] + 1) * (2 * reps[2] + 1);
  XEQ_CHECK_ARG(out_count == 6 * nc + 12, "xeq_pbc_tables_device: out[] holds %lld values, need %lld", (long long)out_count, (long long)(6 * nc + 12));
  Reps3 r;
  for (int k = 0; k < 3; ++k) {
    r.reps[k] = reps[k];
    r.pbc[k] = pbc[k] ? 1 : 0;
  }
  XEQ_DISPATCH_FLOAT(dtype, {
    hipLaunchKernelGGL(k_pbc_tables<T>, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)cell, r, nc, cutoff, (T*)out,
                       reps_needed);
  });
  XEQ_CHECK_LAUNCH("xeq_pbc_tables_device");
  return XEQ_OK;
}

int xeq_npt_front(const xeq_res_system* sys, const xeq_md_params* md, const xeq_npt_params* npt, double dt, void* stream) {
  const char* who = "xeq_npt_front";
  RES_TRY(res_dtype(who, sys, md && npt));
  const int64_t n = sys->n;
  XEQ_CHECK_ARG(n >= 0 && n < RES_MAX_ATOMS, "xeq_npt_front: %lld atoms", (long long)n);
  XEQ_CHECK_ARG(res_finite(dt) && dt >= 0.0, "xeq_npt_front: time step %g", dt);
  XEQ_CHECK_ARG(res_finite(md->dt_over_tau) && md->dt_over_tau >= 0.0 && res_finite(md->t0) && md->t0 >= 0.0,
                "xeq_npt_front: berendsen needs dt / tau >= 0 and a target temperature >= 0 (got %g, %g)", md->dt_over_tau, md->t0);
  XEQ_CHECK_ARG(npt->box && npt->step_cell, "xeq_npt_front: null box record or cell");
  XEQ_CHECK_ARG(n == 0 || (sys->pos && sys->vel && sys->frc && md->inv_mass && sys->image), "xeq_npt_front: null state buffer");
  XEQ_CHECK_ARG(n == 0 || (sys->batch && md->ke && md->tfac), "xeq_npt_front: berendsen needs batch, ke and tfac");
  if (n == 0) return XEQ_OK;
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    MdFrontArgs<T> a{n, 1, dt == 0.0 ? XEQ_MD_NVE : XEQ_MD_BERENDSEN, (T*)sys->pos, (T*)sys->vel, (const T*)sys->frc, (const T*)md->inv_mass, sys->batch,
                     (const T*)md->ke, (const T*)md->tfac, nullptr, nullptr, 0, dt, 1.0, 0.0, md->dt_over_tau, md->t0, sys->image, ResBox{}};
    hipLaunchKernelGGL(k_npt_front<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, npt->box, (T*)npt->step_cell);
  });
  XEQ_CHECK_LAUNCH("xeq_npt_front");
  return XEQ_OK;
}

int xeq_npt_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                 const xeq_npt_params* npt, const xeq_res_recorder* rec, int advance, void* stream) {
  const char* who = "xeq_npt_back";
  RES_TRY(res_dtype(who, sys, step && chunks && md && npt));
  if (!rec) rec = &RES_NO_RECORDER;
  const int64_t n = sys->n, n_chunks = sys->n_chunks;
  XEQ_CHECK_ARG(n >= 1 && n < RES_MAX_ATOMS && n_chunks >= 1 && n_chunks < ((int64_t)1 << 31), "xeq_npt_back: %lld atoms, %lld chunks", (long long)n,
                (long long)n_chunks);
  RES_TRY(res_chunks_hold(who, sys));
  XEQ_CHECK_ARG(res_finite(md->half_dt) && md->half_dt >= 0.0, "xeq_npt_back: half time step %g", md->half_dt);
  XEQ_CHECK_ARG(res_finite(npt->kappa) && npt->kappa >= 0.0 && res_finite(npt->p0) && res_finite(npt->p_unit),
                "xeq_npt_back: barostat (dt / taup * beta / 3 = %g >= 0, target pressure %g, pressure unit %g)", npt->kappa, npt->p0, npt->p_unit);
  RES_TRY(res_recorder(who, rec));
  XEQ_CHECK_ARG(sys->book && step->n_edges_step && npt->box && step->virial_step && npt->virial,
                "xeq_npt_back: null step counter, edge count, box record or virial");
  XEQ_CHECK_ARG(!step->reps_needed || npt->reps_seen, "xeq_npt_back: image counts of the step without the captured counts or the running maximum");
  XEQ_CHECK_ARG(res_back_buffers(sys, step, chunks, true) && md->inv_mass && md->half_mass, "xeq_npt_back: null per-atom or per-chunk buffer");
  XEQ_CHECK_ARG(step->energy_step && chunks->graph_chunk_ptr && md->ke && md->epot, "xeq_npt_back: null per-graph buffer");
  const bool on = advance && rec->every > 0 && rec->rows > 0;
  XEQ_CHECK_ARG(!on || (rec->traj_pos && rec->traj_epot && rec->traj_second && rec->traj_step && rec->traj_cell && rec->traj_pressure && sys->image),
                "xeq_npt_back: null trajectory buffer");
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    ResBox any{};
    any.any = any.periodic[0] = any.periodic[1] = any.periodic[2] = 1;   // (the recorder's cell is the record's: NptBox::cell)
    const MdBackArgs<T> a = md_back_args<T>(sys, step, chunks, md, rec, 1, advance, any, on);
    NptBox<T> bx{(const T*)step->virial_step, (T*)npt->virial, npt->box, step->reps_needed, npt->reps_seen,
                 {(int32_t)step->reps[0], (int32_t)step->reps[1], (int32_t)step->reps[2]}, npt->kappa, npt->p0, npt->p_unit, (T*)rec->traj_cell,
                 rec->traj_pressure};
    hipLaunchKernelGGL(k_npt_back<T>, dim3((unsigned)n_chunks), dim3(MD_CHUNK), 0, (hipStream_t)stream, a, bx);
    XEQ_CHECK_LAUNCH("xeq_npt_back");
    if (n_chunks != 1) hipLaunchKernelGGL(k_npt_join<T>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, bx);
  });
  XEQ_CHECK_LAUNCH("xeq_npt_back");
  return XEQ_OK;
}

// What both thermostat entries ask of their record.
static int nvt_params(const char* who, const xeq_res_system* sys, const xeq_nvt_params* nvt) {
  XEQ_CHECK_ARG(nvt->kind == XEQ_NVT_NOSE_HOOVER || nvt->kind == XEQ_NVT_BUSSI, "%s: thermostat %lld (0 nose-hoover chain, 1 bussi)", who,
                (long long)nvt->kind);
  XEQ_CHECK_ARG(nvt->kind != XEQ_NVT_NOSE_HOOVER || (nvt->chain_length >= 1 && nvt->chain_length <= XEQ_NVT_MAX_CHAIN),
                "%s: chain length %lld (1 .. %d)", who, (long long)nvt->chain_length, XEQ_NVT_MAX_CHAIN);
  XEQ_CHECK_ARG(res_finite(nvt->kT) && nvt->kT > 0.0 && res_finite(nvt->tau) && nvt->tau > 0.0 && res_finite(nvt->dt) && nvt->dt >= 0.0,
                "%s: thermostat (k_B T %g > 0, tau %g > 0, dt %g >= 0)", who, nvt->kT, nvt->tau, nvt->dt);
  XEQ_CHECK_ARG(sys->n_graphs == 0 || (nvt->state && nvt->n_free && (nvt->kind != XEQ_NVT_BUSSI || nvt->graph_rng_id)),
                "%s: null thermostat state, free-atom counts or graph ids", who);
  return XEQ_OK;
}

int xeq_nvt_front(const xeq_res_system* sys, const xeq_md_params* md, const xeq_nvt_params* nvt, double dt, void* stream) {
  const char* who = "xeq_nvt_front";
  RES_TRY(res_dtype(who, sys, md && nvt));
  const int64_t n = sys->n, n_graphs = sys->n_graphs;
  RES_TRY(res_atoms_graphs(who, sys));
  XEQ_CHECK_ARG(res_finite(dt) && dt >= 0.0, "xeq_nvt_front: time step %g", dt);
  RES_TRY(nvt_params(who, sys, nvt));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(n == 0 || (sys->pos && sys->vel && sys->frc && md->inv_mass), "xeq_nvt_front: null state buffer");
  XEQ_CHECK_ARG(n == 0 || !box.any || sys->image, "xeq_nvt_front: a periodic system needs the image counts");
  XEQ_CHECK_ARG(n == 0 || (sys->batch && n_graphs >= 1), "xeq_nvt_front: the factor needs batch and a graph");
  if (n == 0) return XEQ_OK;
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    MdFrontArgs<T> a{n, n_graphs, XEQ_MD_NVE, (T*)sys->pos, (T*)sys->vel, (const T*)sys->frc, (const T*)md->inv_mass, sys->batch, nullptr, nullptr,
                     nullptr, nullptr, 0, dt, 1.0, 0.0, 0.0, 0.0, sys->image, box};
    hipLaunchKernelGGL(k_nvt_front<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, NvtFactor{nvt->state, dt > 0.0});
  });
  XEQ_CHECK_LAUNCH("xeq_nvt_front");
  return XEQ_OK;
}

int xeq_nvt_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                 const xeq_nvt_params* nvt, const xeq_res_recorder* rec, int advance, void* stream) {
  const char* who = "xeq_nvt_back";
  RES_TRY(res_dtype(who, sys, step && chunks && md && nvt));
  if (!rec) rec = &RES_NO_RECORDER;
  const int64_t n = sys->n, n_graphs = sys->n_graphs, n_chunks = sys->n_chunks;
  RES_TRY(res_back_sizes(who, sys, (int64_t)1 << 31));
  XEQ_CHECK_ARG(res_finite(md->half_dt) && md->half_dt >= 0.0, "xeq_nvt_back: half time step %g", md->half_dt);
  RES_TRY(nvt_params(who, sys, nvt));
  RES_TRY(res_recorder(who, rec));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(sys->book && step->n_edges_step, "xeq_nvt_back: null step counter or edge count");
  XEQ_CHECK_ARG(n == 0 || (res_back_buffers(sys, step, chunks, true) && md->inv_mass && md->half_mass), "xeq_nvt_back: null per-atom or per-chunk buffer");
  XEQ_CHECK_ARG(n_graphs == 0 || (step->energy_step && chunks->graph_chunk_ptr && md->ke && md->epot), "xeq_nvt_back: null per-graph buffer");
  const bool on = advance && rec->every > 0 && rec->rows > 0;
  if (on) RES_TRY(res_trajectory(who, sys, rec, box));
  const NvtThermostat th{(int)nvt->kind, (int)nvt->chain_length, nvt->state, nvt->n_free, nvt->graph_rng_id, md->seed, nvt->kT, nvt->tau, nvt->dt};
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    const MdBackArgs<T> a = md_back_args<T>(sys, step, chunks, md, rec, n_graphs, advance, box, on);
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_nvt_back<T>, dim3((unsigned)n_chunks), dim3(MD_CHUNK), 0, (hipStream_t)stream, a, th);
      XEQ_CHECK_LAUNCH("xeq_nvt_back");
    }
    if (n_chunks != 1) hipLaunchKernelGGL(k_nvt_join<T>, dim3(1), dim3(n_graphs > 64 ? MD_JOIN_THREADS : 256), 0, (hipStream_t)stream, a, th);
  });
  XEQ_CHECK_LAUNCH("xeq_nvt_back");
  return XEQ_OK;
}

int xeq_fire_front(const xeq_res_system* sys, const xeq_fire_params* fire, void* stream) {
  const char* who = "xeq_fire_front";
  RES_TRY(res_dtype(who, sys, fire));
  const int64_t n = sys->n, n_graphs = sys->n_graphs;
  RES_TRY(res_atoms_graphs(who, sys));
  RES_TRY(res_in_graph(who, sys));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(n == 0 || (sys->pos && sys->vel && sys->frc && sys->batch && fire->status && fire->coef), "xeq_fire_front: null state buffer");
  XEQ_CHECK_ARG(n == 0 || !box.any || sys->image, "xeq_fire_front: a periodic system needs the image counts");
  if (n == 0) return XEQ_OK;
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    FireFrontArgs<T> a{n, n_graphs, (T*)sys->pos, (T*)sys->vel, (const T*)sys->frc, fire->fixed, sys->batch, fire->status, fire->coef, sys->image, box};
    hipLaunchKernelGGL(k_fire_front<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  });
  XEQ_CHECK_LAUNCH("xeq_fire_front");
  return XEQ_OK;
}

int xeq_fire_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_fire_params* fire,
                  const xeq_res_recorder* rec, void* stream) {
  const char* who = "xeq_fire_back";
  RES_TRY(res_dtype(who, sys, step && chunks && fire));
  if (!rec) rec = &RES_NO_RECORDER;
  const int64_t n = sys->n, n_graphs = sys->n_graphs, n_chunks = sys->n_chunks;
  const xeq_fire_params& f = *fire;
  RES_TRY(res_back_sizes(who, sys, (int64_t)1 << 29));
  RES_TRY(res_in_graph(who, sys));
  XEQ_CHECK_ARG(f.fmax_tol > 0.0 && res_finite(f.fmax_tol), "xeq_fire_back: fmax %g", f.fmax_tol);
  XEQ_CHECK_ARG(f.maxstep > 0.0 && f.dtmax > 0.0 && res_finite(f.maxstep) && res_finite(f.dtmax), "xeq_fire_back: maxstep %g, dtmax %g", f.maxstep,
                f.dtmax);
  XEQ_CHECK_ARG(f.f_inc >= 1.0 && res_finite(f.f_inc) && f.f_dec > 0.0 && f.f_dec < 1.0 && f.alpha_start >= 0.0 && f.alpha_start <= 1.0 &&
                    f.f_alpha > 0.0 && f.f_alpha <= 1.0 && f.n_min >= 0 && f.n_min < ((int64_t)1 << 31),
                "xeq_fire_back: mixing parameters (f_inc %g, f_dec %g, alpha_start %g, f_alpha %g, n_min %lld)", f.f_inc, f.f_dec, f.alpha_start,
                f.f_alpha, (long long)f.n_min);
  RES_TRY(res_recorder(who, rec));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  XEQ_CHECK_ARG(sys->book && step->n_edges_step, "xeq_fire_back: null evaluation counter or edge count");
  XEQ_CHECK_ARG(n == 0 || (res_back_buffers(sys, step, chunks, true) && sys->batch), "xeq_fire_back: null per-atom or per-chunk buffer");
  XEQ_CHECK_ARG(n_graphs == 0 || (step->energy_step && chunks->graph_chunk_ptr && f.epot && f.fmax && f.dt && f.alpha && f.n_pos && f.status &&
                                  f.converged_at && f.coef),
                "xeq_fire_back: null per-graph buffer");
  const bool on = rec->every > 0 && rec->rows > 0;
  if (on) RES_TRY(res_trajectory(who, sys, rec, box));
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    FireBackArgs<T> a{n, n_graphs, n_chunks, (const T*)sys->pos, (const T*)sys->vel, (T*)sys->frc, (const T*)step->frc_step, (const T*)step->energy_step,
                      step->n_edges_step, f.fixed, sys->batch, chunks->chunk_atom0, chunks->chunk_n, chunks->graph_chunk_ptr, chunks->partial,
                      chunks->partial_bad, (T*)f.epot, (T*)f.fmax, f.dt, f.alpha, f.n_pos, f.status, f.converged_at, f.coef, sys->book, f.fmax_tol,
                      f.maxstep, f.dtmax, f.f_inc, f.f_dec, f.alpha_start, f.f_alpha, (int)f.n_min, sys->image, box, on ? rec->every : 0, rec->start,
                      rec->rows, (T*)rec->traj_pos, (T*)rec->traj_epot, (T*)rec->traj_second, rec->traj_step};
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_fire_back<T>, dim3((unsigned)n_chunks), dim3(MD_CHUNK), 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_fire_back");
    }
    if (n_chunks != 1) {
      hipLaunchKernelGGL(k_fire_join<T>, dim3(1), dim3(n_graphs > 64 ? MD_JOIN_THREADS : 256), 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_fire_back");
    }
  });
  return XEQ_OK;
}

}  // extern "C"
