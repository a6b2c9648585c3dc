// Cell tables of the periodic search (include/xeq.h: xeq_pbc_image_counts / xeq_pbc_tables_host / xeq_pbc_tables_device): THE statement
// of their arithmetic, used by the host entries (csrc/xeq_graph.hip) and by the device kernel (csrc/xeq_md.hip), so that a box that lives
// on the device gives the search kernels the bits the host tables give.
// Every operation is rounded once in T, in the order written.  On the host, volatile temporaries keep the compiler from contracting or
// re-associating under -ffp-contract=fast; a device object that uses these functions is built with -ffp-contract=off (csrc/build.py),
// and its f32 divide and square root are the correctly rounded ones (hipcc's default: -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace xeq {

template <typename T>
struct CellGeom {
  T cross[3][3];   // a_1 x a_2, a_2 x a_0, a_0 x a_1
  T vol;
  T recip[3][3];   // cross[ax] / vol
  T inv_min[3];    // |recip[ax]|
};

template <typename T>
__host__ __device__ inline T rnd(T v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return v;
#else
  volatile T t = v;
  return t;
#endif
}

template <typename T>
__host__ __device__ inline void cell_geom(const T* c, CellGeom<T>& g) {   // c: [3][3] row-major, rows = lattice vectors
  const int jj[3] = {1, 2, 0}, kk[3] = {2, 0, 1};
  for (int ax = 0; ax < 3; ++ax) {
    const T* a = c + 3 * jj[ax];
    const T* b = c + 3 * kk[ax];
    g.cross[ax][0] = rnd<T>(rnd<T>(a[1] * b[2]) - rnd<T>(a[2] * b[1]));
    g.cross[ax][1] = rnd<T>(rnd<T>(a[2] * b[0]) - rnd<T>(a[0] * b[2]));
    g.cross[ax][2] = rnd<T>(rnd<T>(a[0] * b[1]) - rnd<T>(a[1] * b[0]));
  }
  T v = rnd<T>(c[0] * g.cross[0][0]);
  v = rnd<T>(v + rnd<T>(c[1] * g.cross[0][1]));
  v = rnd<T>(v + rnd<T>(c[2] * g.cross[0][2]));
  g.vol = v;
  for (int ax = 0; ax < 3; ++ax) {
    T q = T(0);
    for (int j = 0; j < 3; ++j) {
      g.recip[ax][j] = rnd<T>(g.cross[ax][j] / g.vol);
      const T sq = rnd<T>(g.recip[ax][j] * g.recip[ax][j]);
      q = j == 0 ? sq : rnd<T>(q + sq);
    }
    g.inv_min[ax] = rnd<T>(std::sqrt(q));
  }
}

// Images along one periodic axis: ceil(cutoff |recip_ax|), capped (a degenerate cell: caught by the caller's size check).
template <typename T>
__host__ __device__ inline int32_t cell_image_count(const CellGeom<T>& cg, int ax, double cutoff) {
  const T r = std::ceil(rnd<T>((T)cutoff * cg.inv_min[ax]));
  return (r > T(0) && r < T(1 << 20)) ? (int32_t)r : (r > T(0) ? (1 << 20) : 0);
}

// Image k of the table (cartesian_prod order, first axis slowest): its integer triple and its Cartesian offset grid . cell.
template <typename T>
__host__ __device__ inline void cell_table_image(const T* a, const int32_t reps[3], int64_t k, T grid[3], T offs[3]) {
  const int64_t n1 = 2 * reps[1] + 1, n2 = 2 * reps[2] + 1;
  grid[0] = (T)(k / (n1 * n2) - reps[0]);
  grid[1] = (T)((k / n2) % n1 - reps[1]);
  grid[2] = (T)(k % n2 - reps[2]);
  for (int j = 0; j < 3; ++j) {
    T v = rnd<T>(grid[0] * a[j]);
    v = rnd<T>(v + rnd<T>(grid[1] * a[3 + j]));
    v = rnd<T>(v + rnd<T>(grid[2] * a[6 + j]));
    offs[j] = v;
  }
}

// recip [3, 3] and thr [3] of one cell.
template <typename T>
__host__ __device__ inline void cell_table_prune(const CellGeom<T>& cg, double cutoff, T* recip, T* thr) {
  for (int ax = 0; ax < 3; ++ax) {
    for (int j = 0; j < 3; ++j) recip[3 * ax + j] = cg.recip[ax][j];
    thr[ax] = rnd<T>(rnd<T>((T)cutoff * cg.inv_min[ax]) + (T)1e-3);
  }
}

}  // namespace xeq
