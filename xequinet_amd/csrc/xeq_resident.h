// What the sources of the device-resident drivers (xeq_md.hip: dynamics, barostat, FIRE; xeq_lbfgs.hip) share: the box and the wrap, the
// recorder's row rule and its unwrapped-position store, the wave butterflies, the cell's inverse, and the argument checks of the front /
// back entries (include/xeq.h: the records).  These are bit contracts -- a periodic run of any driver wraps and records exactly as the
// others do -- so each is written here once.  Both files are built with -ffp-contract=off (csrc/build.py): the double expressions are the
// ones written, operation by operation.
#pragma once
#include "xeq_common.h"

namespace xeq {

struct ResBox {
  double cell[9];   // rows: lattice vectors
  double inv[9];    // frac_k = sum_j x_j inv[3 j + k]
  int periodic[3];
  int any;
};

// Fractional coordinate by the inverse cell, floor, subtract along the periodic axes; twice, because the rounding of the wrapped coordinate
// to T can land an atom that was a hair below a face exactly ON the opposite face.
template <typename T>
__device__ __forceinline__ void res_wrap(const ResBox& b, double x[3], int32_t img[3]) {
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

// The trajectory row a step fills (-1: none): row (step - record_start) / record_every - 1 of the run's buffers, `step` counted behind it.
__device__ __forceinline__ int64_t res_record_row(int64_t record_every, int64_t record_start, int64_t record_rows, int64_t step_after) {
  if (record_every <= 0) return -1;
  const int64_t d = step_after - record_start;
  if (d <= 0 || d % record_every) return -1;
  const int64_t row = d / record_every - 1;
  return row < record_rows ? row : -1;
}

// Atom i's row of the recorder's positions: unwrapped, pos + image . cell with a periodic axis (`any`), in this operation order
// (resident.py: unwrapped_positions restates it).
template <typename T>
__device__ __forceinline__ void res_store_unwrapped(T* traj_pos, int64_t row, int64_t n, int64_t i, const T* pos, const int32_t* image, int any,
                                                    const double* cell) {
  for (int j = 0; j < 3; ++j) {
    double x = (double)pos[3 * i + j];
    if (any)
      x = x + (((double)image[3 * i] * cell[j] + (double)image[3 * i + 1] * cell[3 + j]) + (double)image[3 * i + 2] * cell[6 + j]);
    traj_pos[(row * n + i) * 3 + j] = (T)x;
  }
}

__device__ __forceinline__ double res_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double res_wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__host__ __device__ __forceinline__ double md_det(const double* c) {
  return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
}

// inv [9] with frac_k = sum_j x_j inv[3 j + k] by the adjugate; -> the determinant (inv is not written unless it is finite and not zero).
__host__ __device__ __forceinline__ double md_inverse(const double* c, double* m) {
  const double det = md_det(c);
  if (!(det != 0.0) || !(det - det == 0.0)) return det;
  m[0] = (c[4] * c[8] - c[5] * c[7]) / det;
  m[1] = (c[2] * c[7] - c[1] * c[8]) / det;
  m[2] = (c[1] * c[5] - c[2] * c[4]) / det;
  m[3] = (c[5] * c[6] - c[3] * c[8]) / det;
  m[4] = (c[0] * c[8] - c[2] * c[6]) / det;
  m[5] = (c[2] * c[3] - c[0] * c[5]) / det;
  m[6] = (c[3] * c[7] - c[4] * c[6]) / det;
  m[7] = (c[1] * c[6] - c[0] * c[7]) / det;
  m[8] = (c[0] * c[4] - c[1] * c[3]) / det;
  return det;
}

// ------------------------------------------------------------------------------------------------------------- host
// finite: not NaN and not an infinity
static inline bool res_finite(double x) { return x - x == 0.0; }

// The box of a HOST cell and its periodic axes (false: the cell is singular or not finite); without either, or without a periodic axis, no box.
static bool res_box_of(const double* cell, const int32_t* pbc, ResBox* b) {
  b->any = 0;
  for (int k = 0; k < 9; ++k) b->cell[k] = b->inv[k] = 0.0;
  for (int k = 0; k < 3; ++k) b->periodic[k] = (cell && pbc && pbc[k]) ? 1 : 0;
  if (!cell || !(b->periodic[0] || b->periodic[1] || b->periodic[2])) return true;
  const double det = md_inverse(cell, b->inv);
  if (!(det != 0.0) || !res_finite(det)) return false;
  for (int k = 0; k < 9; ++k) b->cell[k] = cell[k];
  b->any = 1;
  return true;
}

// The checks the front / back entries share (include/xeq.h: the records), each under the entry's own name `who`.
#define RES_TRY(check)               \
  do {                               \
    if (int e_ = (check)) return e_; \
  } while (0)

static int res_dtype(const char* who, const xeq_res_system* s, bool records) {
  XEQ_CHECK_ARG(s && records, "%s: null argument record", who);
  XEQ_CHECK_ARG(s->dtype == XEQ_F32 || s->dtype == XEQ_F64, "%s: dtype %lld (0 f32, 1 f64)", who, (long long)s->dtype);
  return XEQ_OK;
}

static const int64_t RES_MAX_ATOMS = ((int64_t)1 << 31) / 3;

// A front's sizes.
static int res_atoms_graphs(const char* who, const xeq_res_system* s) {
  XEQ_CHECK_ARG(s->n >= 0 && s->n < RES_MAX_ATOMS && s->n_graphs >= 0, "%s: %lld atoms, %lld graphs", who, (long long)s->n, (long long)s->n_graphs);
  return XEQ_OK;
}

// The minimisers: every atom belongs to a graph.
static int res_in_graph(const char* who, const xeq_res_system* s) {
  XEQ_CHECK_ARG(s->n == 0 || s->n_graphs >= 1, "%s: %lld atoms in no graph", who, (long long)s->n);
  return XEQ_OK;
}

static int res_chunks_hold(const char* who, const xeq_res_system* s) {
  XEQ_CHECK_ARG(s->n_chunks <= s->n && s->n_chunks * XEQ_MD_CHUNK >= s->n, "%s: %lld chunks of at most %d atoms cannot hold %lld atoms", who,
                (long long)s->n_chunks, XEQ_MD_CHUNK, (long long)s->n);
  return XEQ_OK;
}

// A batch's sizes with its chunk count (fewer than `chunk_cap` chunks) ...
static int res_batch_sizes(const char* who, const xeq_res_system* s, int64_t chunk_cap) {
  XEQ_CHECK_ARG(s->n >= 0 && s->n < RES_MAX_ATOMS && s->n_graphs >= 0 && s->n_chunks >= 0 && s->n_chunks < chunk_cap,
                "%s: %lld atoms, %lld graphs, %lld chunks", who, (long long)s->n, (long long)s->n_graphs, (long long)s->n_chunks);
  return XEQ_OK;
}

// ... and a batch's back: those, then the chunk count against the atom count.
static int res_back_sizes(const char* who, const xeq_res_system* s, int64_t chunk_cap) {
  RES_TRY(res_batch_sizes(who, s, chunk_cap));
  return res_chunks_hold(who, s);
}

static int res_recorder(const char* who, const xeq_res_recorder* r) {
  XEQ_CHECK_ARG(r->every >= 0 && r->rows >= 0 && r->start >= 0, "%s: recorder (%lld, %lld, %lld)", who, (long long)r->every, (long long)r->start,
                (long long)r->rows);
  return XEQ_OK;
}

static int res_box(const char* who, const xeq_res_system* s, ResBox* box) {
  XEQ_CHECK_ARG(res_box_of(s->cell, s->pbc, box), "%s: the cell is singular or not finite", who);
  return XEQ_OK;
}

// The buffers every back reads or writes per atom and per chunk; `vel`: the driver has velocities (L-BFGS has none: NULL is taken).
static bool res_back_buffers(const xeq_res_system* s, const xeq_res_step* st, const xeq_res_chunks* c, bool vel) {
  return s->pos && (!vel || s->vel) && s->frc && st->frc_step && c->chunk_atom0 && c->chunk_n && c->partial && c->partial_bad;
}

// The rows of a batch's recorder that is on (xeq_md_back, xeq_fire_back, xeq_lbfgs_back).
static int res_trajectory(const char* who, const xeq_res_system* s, const xeq_res_recorder* r, const ResBox& box) {
  XEQ_CHECK_ARG((s->n == 0 || r->traj_pos) && (s->n_graphs == 0 || (r->traj_epot && r->traj_second)) && r->traj_step, "%s: null trajectory buffer", who);
  XEQ_CHECK_ARG(s->n == 0 || !box.any || s->image, "%s: a periodic system's recorder needs the image counts", who);
  return XEQ_OK;
}

static const xeq_res_recorder RES_NO_RECORDER = {};

}  // namespace xeq
