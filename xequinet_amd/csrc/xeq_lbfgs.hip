// Batched limited-memory BFGS around the whole-step graphs (xequinet_amd/optimize.py: LBFGS): every graph is its
// own minimiser, without line search, by the rule of ASE's optimize.LBFGS.  The contract -- state, arithmetic, summation orders -- is the
// text at xeq_lbfgs_front / xeq_lbfgs_back in include/xeq.h; tests/lbfgs_oracle.py restates it in numpy.  Plain vector code, f32 and f64
// positions and forces; the history, the Gram matrix and the coefficients are double.
//
// The two-loop recursion runs in COEFFICIENT SPACE: the direction is a combination of the basis b = (s_0 .. s_{m-1}, y_0 .. y_{m-1}, g),
// the recursion needs only the dot products of basis vectors (the Gram matrix B, kept per graph and refreshed by three rows per
// evaluation), and the atoms are touched twice per iteration: once to form the new rows' partial dot products (back), once to form the
// direction from the coefficients (front).  Both passes are spread over the chunks of XEQ_MD_CHUNK atoms the other resident drivers use.
//
// Launches.  back = [chunk partials] + [graph: combine in chunk order, decide, ring rows, Gram rows, recursion; books]; front =
// [direction, chunk max |p|^2] + [move, wrap].  When no graph has more than one chunk the workgroup that owns the graph does both halves
// of an entry in one launch.  The workgroup that finishes LAST keeps the books; it is elected by an integer ticket, the file's only
// atomic, and no sum goes through it.  The file is built with -ffp-contract=off (csrc/build.py): the double expressions are the ones
// written here, operation by operation.
#include "xeq_common.h"
#include "xeq_resident.h"

namespace xeq {

constexpr int LB_CHUNK = XEQ_MD_CHUNK;
constexpr int LB_WAVES = LB_CHUNK / 64;
constexpr int LB_MAX_M = XEQ_LBFGS_MAX_MEMORY;
constexpr int LB_MAX_K = 2 * LB_MAX_M + 1;   // basis vectors: s slots, y slots, g
constexpr int LB_GROUP = 4;               // columns of the back's first half whose loads are in flight together
constexpr int LB_MAX_W = 2 * LB_MAX_M + 3;   // columns of a candidate's partial row: s slots, y slots, the candidates s, y, g

template <typename T>
struct LbArgs {
  int64_t n, n_graphs, n_chunks;
  int m;       // memory
  int fused;   // no graph has more than one chunk: one launch per entry
  T* pos;
  T* frc;   // the driver's forces: f_prev until the back has formed y, f behind it
  const T* frc_step;
  const T* energy_step;
  const int32_t* n_edges_step;
  const uint8_t* fixed;
  const int64_t* batch;
  const int32_t* chunk_atom0;
  const int32_t* chunk_n;
  const int32_t* graph_chunk_ptr;
  double* partial;   // [n_chunks, 3 (2 m + 3) + 1]
  int32_t* meta;     // [n_chunks, 4]: the chunk's non-finite flag, its graph's status and head | count << 8 in front of this back; the graph's flag
  double* hist_s;    // [m, n, 3]
  double* hist_y;
  double* pending;   // [n, 3]: the direction between the front's two halves, the displacement s behind it
  double* gram;      // [n_graphs, K, K]
  double* delta;     // [n_graphs, K]
  int32_t* count;
  int32_t* head;
  int32_t* status;
  int32_t* dropped;
  int64_t* converged_at;
  T* epot;
  T* fmax;
  int64_t* book;
  int32_t* ticket;
  double fmax_tol, inv_alpha, maxstep, damping;
  int32_t* image;
  ResBox box;
  int64_t record_every, record_start, record_rows;
  T* traj_pos;
  T* traj_epot;
  T* traj_fmax;
  int64_t* traj_step;
};

__device__ __forceinline__ double lb_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// What every workgroup knows of its chunk: its atoms, its graph and that graph's chunks.
struct LbChunk {
  int cn;
  int64_t i, g, cb, ce;
  bool valid;
};

template <typename T>
__device__ __forceinline__ LbChunk lb_chunk(const LbArgs<T>& a, int64_t c) {
  LbChunk k;
  int cn = a.chunk_n[c];
  k.cn = cn < 0 ? 0 : (cn > LB_CHUNK ? LB_CHUNK : cn);
  int64_t a0 = a.chunk_atom0[c];
  a0 = a0 < 0 ? 0 : (a0 >= a.n ? a.n - 1 : a0);
  k.i = a0 + threadIdx.x;
  k.valid = (int)threadIdx.x < k.cn && k.i < a.n;
  int64_t g = a.batch[a0];
  k.g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);
  if (a.fused) {
    k.cb = c;
    k.ce = c + 1;
  } else {
    int64_t cb = a.graph_chunk_ptr[k.g], ce = a.graph_chunk_ptr[k.g + 1];
    k.cb = cb < 0 ? 0 : (cb > c ? c : cb);
    k.ce = ce > a.n_chunks ? a.n_chunks : (ce <= c ? c + 1 : ce);
  }
  return k;
}

// --------------------------------------------------------------------------------------------------------------- back, first half
// One workgroup per chunk: the partial dot products of the three candidate vectors -- the pending s, y = f_prev - f, g = -f, zero for a
// fixed atom -- with every stored s_j and y_j and with one another, and max |f_i|^2: lanes, butterfly, the four waves in order.
template <typename T>
__device__ __forceinline__ void lb_back_chunk(const LbArgs<T>& a, int64_t c, double (*wsum)[LB_WAVES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.m, W = 2 * m + 3, PS = 3 * W + 1;
  const LbChunk k = lb_chunk(a, c);
  const int st = a.status[k.g];
  int cnt = a.count[k.g], hd = a.head[k.g];
  cnt = cnt < 0 ? 0 : (cnt > m ? m : cnt);
  hd = hd < 0 ? 0 : (hd >= m ? m - 1 : hd);
  const bool frozen = st == XEQ_LBFGS_CONVERGED;
  double cand[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  int bad = 0;
  const int64_t i = k.i;
  if (k.valid) {
    const bool fix = a.fixed && a.fixed[i];
    for (int j = 0; j < 3; ++j) {
      const T fk = a.frc_step[3 * i + j];
      bad |= !isfinite((double)fk);
      const double f = fix ? 0.0 : (double)fk;
      cand[2][j] = -f;
      if (st == XEQ_LBFGS_ACTIVE && !fix) {
        cand[0][j] = a.pending[3 * i + j];
        cand[1][j] = (double)a.frc[3 * i + j] - f;
      }
    }
    const int64_t row = res_record_row(a.record_every, a.record_start, a.record_rows, a.book[0]);
    if (row >= 0) res_store_unwrapped(a.traj_pos, row, a.n, i, a.pos, a.image, a.box.any, a.box.cell);
  }
  const int any_bad = __syncthreads_or(bad);
  if (!frozen) {
    // LB_GROUP columns at a time: their loads are issued together, then their 3 LB_GROUP independent reductions (the sums and their
    // orders are those of one column after the other)
    for (int c0 = 0; c0 < W; c0 += LB_GROUP) {
      double b[LB_GROUP][3];
      bool empty[LB_GROUP];
#pragma unroll
      for (int u = 0; u < LB_GROUP; ++u) {
        const int col = c0 + u;
        const bool slot = col < 2 * m;
        const int j = col < m ? col : col - m;
        empty[u] = slot && j >= cnt;   // an empty slot: no loads, zeros
        for (int x = 0; x < 3; ++x) b[u][x] = 0.0;
        if (col < W && k.valid && !empty[u]) {
          if (slot) {
            const double* h = (col < m ? a.hist_s : a.hist_y) + ((int64_t)j * a.n + i) * 3;
            for (int x = 0; x < 3; ++x) b[u][x] = h[x];
          } else {
            const int which = col - 2 * m;
            for (int x = 0; x < 3; ++x) b[u][x] = which == 0 ? cand[0][x] : (which == 1 ? cand[1][x] : cand[2][x]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < LB_GROUP; ++u) {
        const int col = c0 + u;
        if (col >= W) break;
        for (int q = 0; q < 3; ++q) {
          const double v = res_wave_sum(lb_dot(cand[q], b[u]));
          if (lane == 0) wsum[q * W + col][wave] = empty[u] ? 0.0 : v;
        }
      }
    }
    const double m2 = res_wave_max(lb_dot(cand[2], cand[2]));
    if (lane == 0) wsum[3 * W][wave] = m2;
  }
  __syncthreads();
  if (!frozen) {
    for (int q = tid; q < PS; q += LB_CHUNK) {
      double s = wsum[q][0];
      for (int w = 1; w < LB_WAVES; ++w) s = q == 3 * W ? fmax(s, wsum[q][w]) : s + wsum[q][w];
      a.partial[c * PS + q] = s;
    }
  }
  if (tid == 0) {
    a.meta[4 * c] = (any_bad && !frozen) ? 1 : 0;
    a.meta[4 * c + 1] = st;
    a.meta[4 * c + 2] = hd | (cnt << 8);
  }
}

// --------------------------------------------------------------------------------------------------------------- back, second half
// Every workgroup of a graph adds the graph's partials in chunk order (the same loop, so the same bits) and takes the same decisions;
// it writes its own atoms' rows of the ring and of frc.  The workgroup of the graph's FIRST chunk refreshes the Gram rows, runs the
// recursion (wave 0: lane l holds delta_l and delta_{64 + l}; a row product is B[r, l] delta_l + B[r, 64 + l] delta_{64 + l} per lane
// and a butterfly) and stores the graph's state.
template <typename T>
__device__ __forceinline__ void lb_back_graph(const LbArgs<T>& a, int64_t c, double* tot, double* Bl, int* sflag) {
  const int tid = threadIdx.x;
  const int m = a.m, K = 2 * m + 1, W = 2 * m + 3, PS = 3 * W + 1;
  const LbChunk k = lb_chunk(a, c);
  const int64_t g = k.g, i = k.i;
  const bool first = c == k.cb;
  const int st = a.meta[4 * c + 1], hd = a.meta[4 * c + 2] & 255, cnt = a.meta[4 * c + 2] >> 8;
  const int64_t eval = a.book[0];
  const int64_t row = res_record_row(a.record_every, a.record_start, a.record_rows, eval);
  if (st == XEQ_LBFGS_CONVERGED) {   // left alone, bit for bit; only its recorder row is filled, from what it kept
    if (first && tid == 0) {
      a.meta[4 * c + 3] = 0;
      if (row >= 0) {
        a.traj_epot[row * a.n_graphs + g] = a.epot[g];
        a.traj_fmax[row * a.n_graphs + g] = a.fmax[g];
      }
    }
    return;
  }
  for (int q = tid; q < PS; q += LB_CHUNK) {
    double s = a.partial[k.cb * PS + q];
    for (int64_t cc = k.cb + 1; cc < k.ce; ++cc) s = q == 3 * W ? fmax(s, a.partial[cc * PS + q]) : s + a.partial[cc * PS + q];
    tot[q] = s;
  }
  if (tid == 0) {
    int b = 0;
    for (int64_t cc = k.cb; cc < k.ce; ++cc) b |= a.meta[4 * cc];
    *sflag = b;
  }
  __syncthreads();
  const double fm = sqrt(tot[3 * W]);
  const bool conv = fm < a.fmax_tol;
  const double sy = tot[2 * m + 1];   // s . y of the candidates
  const bool accept = st == XEQ_LBFGS_ACTIVE && !conv && isfinite(sy) && sy > 0.0;
  if (k.valid) {
    const bool fix = a.fixed && a.fixed[i];
    for (int j = 0; j < 3; ++j) {
      const T fk = a.frc_step[3 * i + j];
      if (accept) {
        const int64_t at = ((int64_t)hd * a.n + i) * 3 + j;
        a.hist_s[at] = fix ? 0.0 : a.pending[3 * i + j];
        a.hist_y[at] = fix ? 0.0 : (double)a.frc[3 * i + j] - (double)fk;
      }
      a.frc[3 * i + j] = fix ? T(0) : fk;
    }
  }
  if (!first) return;
  const T e = a.energy_step[g];
  if (tid == 0) {
    a.meta[4 * c + 3] = (*sflag || !isfinite((double)e)) ? 1 : 0;
    a.epot[g] = e;
    a.fmax[g] = (T)fm;
    if (row >= 0) {
      a.traj_epot[row * a.n_graphs + g] = e;
      a.traj_fmax[row * a.n_graphs + g] = (T)fm;
    }
  }
  if (conv) {
    if (tid == 0) {
      a.status[g] = XEQ_LBFGS_CONVERGED;
      a.converged_at[g] = eval;
    }
    return;
  }
  const int cnt2 = accept ? (cnt + 1 > m ? m : cnt + 1) : cnt;
  const int hd2 = accept ? (hd + 1) % m : hd;
  double* Bg = a.gram + g * (int64_t)(K * K);
  for (int q = accept ? 0 : 2; q < 3; ++q) {   // the new pair's rows against everything stored, g's row against everything
    const int r = q == 0 ? hd : (q == 1 ? m + hd : 2 * m);
    for (int t = tid; t < K; t += LB_CHUNK) {
      const int j = t < m ? t : t - m;
      const bool ok = t == 2 * m || j < cnt2;
      int col = t == 2 * m ? 2 * m + 2 : t;
      if (accept && t < 2 * m && j == hd) col = t < m ? 2 * m : 2 * m + 1;
      if (ok) {
        const double v = tot[q * W + col];
        Bg[r * K + t] = v;
        Bg[t * K + r] = v;
      }
    }
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  for (int q = tid; q < K * K; q += LB_CHUNK) Bl[q] = Bg[q];
  __syncthreads();
  if (tid < 64) {
    const int l = tid, k0 = l, k1 = 64 + l;
    auto live = [&](int x) { return x < K && (x == 2 * m || (x < m ? x : x - m) < cnt2); };
    const bool on0 = live(k0), on1 = live(k1);
    double d0 = k0 == 2 * m ? 1.0 : 0.0, d1 = k1 == 2 * m ? 1.0 : 0.0;   // delta = e_g
    double a_mine = 0.0;                                                  // lane `slot` keeps a_slot
    auto rowdot = [&](int r) {
      double t = on0 ? Bl[r * K + k0] * d0 : 0.0;
      if (on1) t = t + Bl[r * K + k1] * d1;
      return res_wave_sum(t);
    };
    for (int t = 0; t < cnt2; ++t) {   // newest to oldest
      const int slot = (hd2 - 1 - t + 2 * m) % m;
      const double ai = rowdot(slot) / Bl[slot * K + m + slot];
      if (l == slot) a_mine = ai;
      if (l == m + slot) d0 = d0 - ai;   // (m + slot < 64 for every memory up to 32)
    }
    d0 = d0 * a.inv_alpha;
    d1 = d1 * a.inv_alpha;
    for (int t = cnt2 - 1; t >= 0; --t) {   // oldest to newest
      const int slot = (hd2 - 1 - t + 2 * m) % m;
      const double beta = rowdot(m + slot) / Bl[slot * K + m + slot];
      const double ai = __shfl(a_mine, slot, 64);
      if (l == slot) d0 = d0 + (ai - beta);
    }
    if (k0 < K) a.delta[g * K + k0] = on0 ? d0 : 0.0;
    if (k1 < K) a.delta[g * K + k1] = on1 ? d1 : 0.0;
    if (l == 0) {
      if (st == XEQ_LBFGS_ACTIVE && !accept) a.dropped[g] = a.dropped[g] + 1;
      a.count[g] = cnt2;
      a.head[g] = hd2;
      a.status[g] = XEQ_LBFGS_ACTIVE;
    }
  }
}

// The workgroup that takes the last ticket keeps the books: the graphs without atoms (they converge at their first evaluation), the
// flag, the count of graphs that are not converged, the four integers.
template <typename T>
__device__ __forceinline__ void lb_books(const LbArgs<T>& a, int* slast) {
  const int tid = threadIdx.x;
  __threadfence();
  __syncthreads();
  if (tid == 0) *slast = atomicAdd(a.ticket, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!*slast) return;
  __threadfence();
  const int64_t eval = a.book[0];
  const int64_t row = res_record_row(a.record_every, a.record_start, a.record_rows, eval);
  int bad = 0;
  int64_t active = 0;
  for (int64_t base = 0; base < a.n_graphs; base += LB_CHUNK) {
    const int64_t g = base + tid;
    int open = 0;
    if (g < a.n_graphs) {
      int64_t cb = a.graph_chunk_ptr[g], ce = a.graph_chunk_ptr[g + 1];
      if (cb >= ce || cb < 0 || cb >= a.n_chunks) {   // no atoms: fmax = 0
        if (a.status[g] != XEQ_LBFGS_CONVERGED) {
          const T e = a.energy_step[g];
          bad |= !isfinite((double)e);
          a.epot[g] = e;
          a.fmax[g] = T(0);
          a.status[g] = XEQ_LBFGS_CONVERGED;
          a.converged_at[g] = eval;
        }
        if (row >= 0) {
          a.traj_epot[row * a.n_graphs + g] = a.epot[g];
          a.traj_fmax[row * a.n_graphs + g] = a.fmax[g];
        }
      } else {
        bad |= __hip_atomic_load(a.meta + 4 * cb + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        open = __hip_atomic_load(a.status + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != XEQ_LBFGS_CONVERGED;
      }
    }
    active += __syncthreads_count(open);
  }
  const int any_bad = __syncthreads_or(bad);
  if (tid == 0) {
    const int64_t ne = (int64_t)a.n_edges_step[0];
    a.book[0] = eval + 1;
    if (ne > a.book[1]) a.book[1] = ne;
    if (any_bad) a.book[2] = 1;
    a.book[3] = active;
    if (row >= 0) a.traj_step[row] = eval;
    *a.ticket = 0;
  }
}

struct LbBackShared {
  double wsum[3 * LB_MAX_W + 1][LB_WAVES];
  double tot[3 * LB_MAX_W + 1];
  double Bl[LB_MAX_K * LB_MAX_K];
  int flag, last;
};

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_back_chunk(LbArgs<T> a) {
  __shared__ double wsum[3 * LB_MAX_W + 1][LB_WAVES];
  if ((int64_t)blockIdx.x < a.n_chunks) lb_back_chunk(a, (int64_t)blockIdx.x, wsum);
}

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_back_graph(LbArgs<T> a) {
  __shared__ double tot[3 * LB_MAX_W + 1];
  __shared__ double Bl[LB_MAX_K * LB_MAX_K];
  __shared__ int flag, last;
  if ((int64_t)blockIdx.x < a.n_chunks) lb_back_graph(a, (int64_t)blockIdx.x, tot, Bl, &flag);
  lb_books(a, &last);
}

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_back_fused(LbArgs<T> a) {
  __shared__ LbBackShared s;
  if ((int64_t)blockIdx.x < a.n_chunks) {
    lb_back_chunk(a, (int64_t)blockIdx.x, s.wsum);
    __threadfence_block();
    __syncthreads();
    lb_back_graph(a, (int64_t)blockIdx.x, s.tot, s.Bl, &s.flag);
  }
  lb_books(a, &s.last);
}

// --------------------------------------------------------------------------------------------------------------- front
// First half, per free atom of an ACTIVE graph: p_i = -sum_k delta_k b_{k,i} in slot order (the stored s slots, the stored y slots, g)
// into `pending`, and the chunk's max |p_i|^2 (lanes, butterfly, the four waves in order) into the chunk's first partial.
template <typename T>
__device__ __forceinline__ void lb_front_direction(const LbArgs<T>& a, int64_t c, double* wmax) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.m, K = 2 * m + 1, PS = 3 * (2 * m + 3) + 1;
  const LbChunk k = lb_chunk(a, c);
  if (a.status[k.g] != XEQ_LBFGS_ACTIVE) return;   // (the whole workgroup: the status is the graph's)
  int cnt = a.count[k.g];
  cnt = cnt < 0 ? 0 : (cnt > m ? m : cnt);
  const double* d = a.delta + k.g * K;
  double p2 = 0.0;
  const int64_t i = k.i;
  if (k.valid && !(a.fixed && a.fixed[i])) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < cnt; ++j) {
      const double* h = a.hist_s + ((int64_t)j * a.n + i) * 3;
      for (int x = 0; x < 3; ++x) acc[x] = acc[x] + d[j] * h[x];
    }
    for (int j = 0; j < cnt; ++j) {
      const double* h = a.hist_y + ((int64_t)j * a.n + i) * 3;
      for (int x = 0; x < 3; ++x) acc[x] = acc[x] + d[m + j] * h[x];
    }
    double p[3];
    for (int x = 0; x < 3; ++x) {
      acc[x] = acc[x] + d[2 * m] * (-(double)a.frc[3 * i + x]);
      p[x] = -acc[x];
      a.pending[3 * i + x] = p[x];
    }
    p2 = lb_dot(p, p);
  }
  p2 = res_wave_max(p2);
  if (lane == 0) wmax[wave] = p2;
  __syncthreads();
  if (tid == 0) {
    double s = wmax[0];
    for (int w = 1; w < LB_WAVES; ++w) s = fmax(s, wmax[w]);
    a.partial[c * PS] = s;
  }
}

// Second half: longest = sqrt(max over the graph's chunks), the clamp, x_new = dtype(x + (damping scale) p), the pending
// s = (double)x_new - (double)x taken BEFORE the wrap, the wrap.
template <typename T>
__device__ __forceinline__ void lb_front_move(const LbArgs<T>& a, int64_t c) {
  const int m = a.m, PS = 3 * (2 * m + 3) + 1;
  const LbChunk k = lb_chunk(a, c);
  if (a.status[k.g] != XEQ_LBFGS_ACTIVE) return;
  double l2 = a.partial[k.cb * PS];
  for (int64_t cc = k.cb + 1; cc < k.ce; ++cc) l2 = fmax(l2, a.partial[cc * PS]);
  const double longest = sqrt(l2);
  const double scale = longest >= a.maxstep ? a.maxstep / longest : 1.0;
  const double step = a.damping * scale;
  const int64_t i = k.i;
  if (!k.valid || (a.fixed && a.fixed[i])) return;
  double x[3];
  for (int j = 0; j < 3; ++j) {
    const double x0 = (double)a.pos[3 * i + j];
    x[j] = (double)(T)(x0 + step * a.pending[3 * i + j]);
    a.pending[3 * i + j] = x[j] - x0;
  }
  if (a.box.any) {
    int32_t img[3] = {a.image[3 * i], a.image[3 * i + 1], a.image[3 * i + 2]};
    res_wrap<T>(a.box, x, img);
    for (int j = 0; j < 3; ++j) a.image[3 * i + j] = img[j];
  }
  for (int j = 0; j < 3; ++j) a.pos[3 * i + j] = (T)x[j];
}

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_front_direction(LbArgs<T> a) {
  __shared__ double wmax[LB_WAVES];
  lb_front_direction(a, (int64_t)blockIdx.x, wmax);
}

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_front_move(LbArgs<T> a) {
  lb_front_move(a, (int64_t)blockIdx.x);
}

template <typename T>
__global__ void __launch_bounds__(LB_CHUNK) k_lbfgs_front_fused(LbArgs<T> a) {
  __shared__ double wmax[LB_WAVES];
  lb_front_direction(a, (int64_t)blockIdx.x, wmax);
  __threadfence_block();
  __syncthreads();
  lb_front_move(a, (int64_t)blockIdx.x);
}

// --------------------------------------------------------------------------------------------------------------- host
// What both entries ask of the memory and of what it makes of the chunk count; `who`: the entry's name.
static int lb_memory(const char* who, const xeq_res_system* s, const xeq_lbfgs_params* p) {
  XEQ_CHECK_ARG(p->memory >= 1 && p->memory <= XEQ_LBFGS_MAX_MEMORY, "%s: memory %lld (1 .. XEQ_LBFGS_MAX_MEMORY = %d)", who, (long long)p->memory,
                XEQ_LBFGS_MAX_MEMORY);
  XEQ_CHECK_ARG(p->max_graph_chunks >= 0 && p->max_graph_chunks <= s->n_chunks, "%s: at most %lld chunks in a graph, of %lld chunks", who,
                (long long)p->max_graph_chunks, (long long)s->n_chunks);
  XEQ_CHECK_ARG(s->n_chunks * (3 * (2 * p->memory + 3) + 1) < ((int64_t)1 << 31) && s->n * p->memory * 3 < ((int64_t)1 << 40),
                "%s: %lld chunks with memory %lld: the partial sums do not fit", who, (long long)s->n_chunks, (long long)p->memory);
  return XEQ_OK;
}

// The kernel arguments both entries fill alike; the back adds the step's outputs, its own state and the recorder.
template <typename T>
static LbArgs<T> lb_args(const xeq_res_system* sys, const xeq_res_chunks* chunks, const xeq_lbfgs_params* p, const ResBox& box) {
  LbArgs<T> a{};
  a.n = sys->n, a.n_graphs = sys->n_graphs, a.n_chunks = sys->n_chunks, a.m = (int)p->memory, a.fused = p->max_graph_chunks <= 1;
  a.pos = (T*)sys->pos, a.frc = (T*)sys->frc, a.fixed = p->fixed, a.batch = sys->batch;
  a.chunk_atom0 = chunks->chunk_atom0, a.chunk_n = chunks->chunk_n, a.graph_chunk_ptr = chunks->graph_chunk_ptr, a.partial = chunks->partial;
  a.hist_s = p->hist_s, a.hist_y = p->hist_y, a.pending = p->pending_s, a.delta = p->delta;
  a.count = p->count, a.status = p->status, a.image = sys->image, a.box = box;
  return a;
}

}  // namespace xeq

using namespace xeq;

extern "C" {

int xeq_lbfgs_front(const xeq_res_system* sys, const xeq_res_chunks* chunks, const xeq_lbfgs_params* lbfgs, void* stream) {
  const char* who = "xeq_lbfgs_front";
  RES_TRY(res_dtype(who, sys, chunks && lbfgs));
  const xeq_lbfgs_params& p = *lbfgs;
  RES_TRY(res_batch_sizes(who, sys, (int64_t)1 << 29));
  RES_TRY(res_in_graph(who, sys));
  RES_TRY(res_chunks_hold(who, sys));
  RES_TRY(lb_memory(who, sys, lbfgs));
  XEQ_CHECK_ARG(p.maxstep > 0.0 && res_finite(p.maxstep), "%s: maxstep %g", who, p.maxstep);
  XEQ_CHECK_ARG(p.damping > 0.0 && res_finite(p.damping), "%s: damping %g", who, p.damping);
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  const int64_t n = sys->n;
  XEQ_CHECK_ARG(n == 0 || (sys->pos && sys->frc && sys->batch && chunks->chunk_atom0 && chunks->chunk_n && chunks->graph_chunk_ptr &&
                           chunks->partial && p.hist_s && p.hist_y && p.pending_s && p.delta && p.count && p.status),
                "%s: null state buffer", who);
  XEQ_CHECK_ARG(n == 0 || !box.any || sys->image, "%s: a periodic system needs the image counts", who);
  if (n == 0) return XEQ_OK;
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    LbArgs<T> a = lb_args<T>(sys, chunks, lbfgs, box);
    a.maxstep = p.maxstep, a.damping = p.damping;
    const dim3 grid((unsigned)sys->n_chunks), block(LB_CHUNK);
    if (a.fused) {
      hipLaunchKernelGGL(k_lbfgs_front_fused<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_front");
    } else {
      hipLaunchKernelGGL(k_lbfgs_front_direction<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_front");
      hipLaunchKernelGGL(k_lbfgs_front_move<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_front");
    }
  });
  return XEQ_OK;
}

int xeq_lbfgs_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_lbfgs_params* lbfgs,
                   const xeq_res_recorder* rec, void* stream) {
  const char* who = "xeq_lbfgs_back";
  RES_TRY(res_dtype(who, sys, step && chunks && lbfgs));
  if (!rec) rec = &RES_NO_RECORDER;
  const xeq_lbfgs_params& p = *lbfgs;
  RES_TRY(res_batch_sizes(who, sys, (int64_t)1 << 29));
  RES_TRY(res_in_graph(who, sys));
  RES_TRY(res_chunks_hold(who, sys));
  RES_TRY(lb_memory(who, sys, lbfgs));
  XEQ_CHECK_ARG(p.fmax_tol > 0.0 && res_finite(p.fmax_tol), "%s: fmax %g", who, p.fmax_tol);
  XEQ_CHECK_ARG(p.alpha > 0.0 && res_finite(p.alpha), "%s: alpha %g", who, p.alpha);
  RES_TRY(res_recorder(who, rec));
  ResBox box;
  RES_TRY(res_box(who, sys, &box));
  const int64_t n = sys->n, n_graphs = sys->n_graphs;
  XEQ_CHECK_ARG(sys->book && step->n_edges_step && p.ticket, "%s: null evaluation counter, edge count or ticket", who);
  XEQ_CHECK_ARG(n == 0 || (res_back_buffers(sys, step, chunks, false) && sys->batch && p.hist_s && p.hist_y && p.pending_s),
                "%s: null per-atom or per-chunk buffer", who);
  XEQ_CHECK_ARG(n_graphs == 0 || (step->energy_step && chunks->graph_chunk_ptr && p.gram && p.delta && p.count && p.head && p.status && p.dropped &&
                                  p.converged_at && p.epot && p.fmax),
                "%s: null per-graph buffer", who);
  const bool on = rec->every > 0 && rec->rows > 0;
  if (on) RES_TRY(res_trajectory(who, sys, rec, box));
  XEQ_DISPATCH_FLOAT(sys->dtype, {
    LbArgs<T> a = lb_args<T>(sys, chunks, lbfgs, box);
    a.frc_step = (const T*)step->frc_step, a.energy_step = (const T*)step->energy_step, a.n_edges_step = step->n_edges_step;
    a.meta = chunks->partial_bad, a.gram = p.gram, a.head = p.head, a.dropped = p.dropped, a.converged_at = p.converged_at;
    a.epot = (T*)p.epot, a.fmax = (T*)p.fmax, a.book = sys->book, a.ticket = p.ticket, a.fmax_tol = p.fmax_tol, a.inv_alpha = 1.0 / p.alpha;
    a.record_every = on ? rec->every : 0, a.record_start = rec->start, a.record_rows = rec->rows;
    a.traj_pos = (T*)rec->traj_pos, a.traj_epot = (T*)rec->traj_epot, a.traj_fmax = (T*)rec->traj_second, a.traj_step = rec->traj_step;
    const dim3 grid((unsigned)(sys->n_chunks > 0 ? sys->n_chunks : 1)), block(LB_CHUNK);
    if (a.fused) {
      hipLaunchKernelGGL(k_lbfgs_back_fused<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_back");
    } else {
      hipLaunchKernelGGL(k_lbfgs_back_chunk<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_back");
      hipLaunchKernelGGL(k_lbfgs_back_graph<T>, grid, block, 0, (hipStream_t)stream, a);
      XEQ_CHECK_LAUNCH("xeq_lbfgs_back");
    }
  });
  return XEQ_OK;
}

}  // extern "C"
