/* libxeq_hip.so -- C ABI of the MI355X-native XPaiNN energy+force hot path.
 *
 * Drop-in boundary.  The reference (X1X1010/XequiNet) is pure
 * Python and has no FFI; its hot path bottoms out in third-party extension ops.
 * Each entry point below names the reference call site it replaces
 * (paths relative to /root/reference/xequinet/).  INTEGRATION.md shows the
 * ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    marked "host".  All buffers are owned by the caller (e.g. the PyTorch
 *    caching allocator); the library never allocates, frees or retains them.
 *  - Row-major contiguous tensors.  `dtype` selects f32/f64 for all floating
 *    tensors of a call.  Index tensors are int64 where the reference's are
 *    (edge_index, ptr), int32 for the library's own CSR arrays.
 *  - Every call enqueues on `stream` (a hipStream_t passed as void*) and
 *    returns without synchronising; re-entrant, no global mutable state
 *    besides the thread-local error string.
 *  - Return value: 0 = ok, otherwise an XEQ_ERR_* code; xeq_last_error()
 *    returns the message for the calling thread (the reference raises Python
 *    exceptions/asserts, e.g. nn/rbf.py:44-46, nn/o3layer.py:105-107).
 *  - Irreps are passed as mul[3] = channels of l = 0,1,2 (0 = absent), e3nn
 *    mul_ir layout; C = sum mul, D = mul0 + 3 mul1 + 5 mul2.
 */
#ifndef XEQ_H
#define XEQ_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { XEQ_F32 = 0, XEQ_F64 = 1 };
/* radial bases of nn/rbf.py: SphericalBesselj0 (p0 = freq), GaussianSmearing (p0 = mean, p1 = std), ExponentialBernstein (p0 =
 * softplus(_alpha) repeated num_basis times, p1 = the log binomials `logc`; nn/rbf.py:161-191), ExponentialNorm (p0 = beta, p1 = mu;
 * nn/rbf.py:194-207).  The last two: inference entry points (xeq_radial_fwd, xeq_edge_basis, xeq_edge_basis_wq, xeq_message_fwd / _bwd);
 * the parameter-gradient kernels of the native training pass take the first two only. */
enum { XEQ_RBF_BESSEL = 0, XEQ_RBF_GAUSSIAN = 1, XEQ_RBF_EXPBERN = 2, XEQ_RBF_EXPNORM = 3 };
enum { XEQ_CUTOFF_COSINE = 0, XEQ_CUTOFF_POLYNOMIAL = 1 };
enum {
  XEQ_OK = 0,
  XEQ_ERR_INVALID_ARGUMENT = 1,
  XEQ_ERR_LAUNCH = 2,
  XEQ_ERR_UNSUPPORTED = 3
};

int xeq_version(void);
const char* xeq_last_error(void);
/* Kernel launches this library has enqueued so far in the process (all threads, every entry point, whichever front called it).
 * Test infrastructure: tests/test_gpu_parity.py::_aten_only proves with it that the ATen-only evaluation of the reference's op
 * sequence -- a member of the fp32 error envelope -- launched no kernel of this library. */
int64_t xeq_launch_count(void);
/* The entry-point names of launches number first .. xeq_launch_count() - 1, one per line, into buf (NUL-terminated).  -> the bytes needed
 * (call with buf = NULL to size it); -1 when `first` is out of range or older than the last 8 192 launches.  Test infrastructure:
 * tests/test_gpu_interface.py compares the launch SEQUENCES of the two fronts (Python modules, xeq::xpainn_eval) with it. */
int64_t xeq_launch_names(int64_t first, char* buf, int64_t cap);

/* ------------------------------------------------------------------ graph */

/* rowptr[i] = first position p with keys[p] >= i, i in [0, n_rows]  (keys sorted
 * ascending).  Turns a destination-sorted edge_index row into CSR. */
int xeq_csr_rowptr(const int64_t* keys, int64_t n_keys, int64_t n_rows, int32_t* rowptr, void* stream);

/* CSR view of an UNSORTED index row (edge_index[1] for the reverse pass, edge_index[0] of a user-built edge list):
 * perm[E] = stable order of the edges by key (a radix sort: ties keep edge order, deterministic), rowptr[n_rows+1] over
 * the sorted keys.  Replaces the stable torch.sort + searchsorted plumbing with one call; `workspace` is a device
 * scratch buffer of at least xeq_csr_by_key_workspace(n_keys, n_rows) bytes (-1: sizes out of range). */
int64_t xeq_csr_by_key_workspace(int64_t n_keys, int64_t n_rows);
int xeq_csr_by_key(const int64_t* keys, int64_t n_keys, int64_t n_rows, void* workspace, int64_t workspace_bytes,
                   int32_t* rowptr, int32_t* perm, void* stream);
/* The same for a CAPACITY-sized key array whose first *n_valid entries are edges (n_valid: device pointer, e.g. the last entry of the
 * center row pointer of a list written without reading its size back): the slots behind them sort to the end as row n_rows, so
 * rowptr[n_rows] = *n_valid and no walk reaches them.  Workspace: xeq_csr_by_key_workspace(n_keys, n_rows + 1).  What lets a
 * periodic neighbour list and its reverse view sit inside one captured HIP graph (runtime.GraphedStepPBC). */
int xeq_csr_by_key_bounded(const int64_t* keys, int64_t n_keys, int64_t n_rows, const int32_t* n_valid, void* workspace,
                           int64_t workspace_bytes, int32_t* rowptr, int32_t* perm, void* stream);

/* Exclusive prefix sum of int32 counts[n] into out[n+1] (out[n] = total). */
int xeq_exclusive_scan_i32(const int32_t* counts, int64_t n, int32_t* out, void* stream);
/* The same scan grid-wide (decoupled look-back), for large n; `workspace`: device scratch of at least
 * xeq_exclusive_scan_i32_workspace(n) bytes (-1: n out of range).  The form above runs in ONE workgroup and needs none. */
int64_t xeq_exclusive_scan_i32_workspace(int64_t n);
int xeq_exclusive_scan_i32_ws(const int32_t* counts, int64_t n, int32_t* out, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* Everything the periodic search derives from the cells alone (HOST function: host pointers in and out, no device work).
 * Replaces the host-side preparation of data/radius_graph.py: images per axis reps[a] = max_g ceil(cutoff |a_j x a_k| / V)
 * on the periodic axes, 0 on the open ones (:61-89); the image table grid[n_cells, 3] in cartesian_prod order, first axis
 * slowest (:93-97); its Cartesian offsets offs[G, n_cells, 3] = grid cell[g] (:98-104); and, for the image-pruned kernels
 * below, recip[G, 3, 3] = rows a_j x a_k / V and thr[G, 3] = cutoff |recip_a| + 1e-3.  Arithmetic in the cells' own dtype
 * with every operation rounded once (no contraction), in the order written here, so that every caller -- the Python front
 * (data/radius_graph.py of this package) and the registered operator xeq::radius_graph_pbc -- hands the search kernels the
 * same bits.  Two phases: xeq_pbc_image_counts gives reps (n_cells = prod (2 reps + 1)); xeq_pbc_tables_host fills
 * out[] = grid | offs | recip | thr, (3 + 3 G) n_cells + 12 G values of `dtype`. */
int xeq_pbc_image_counts(int dtype, const void* cell_host, int64_t n_graphs, const int32_t pbc[3], double cutoff, int32_t reps[3]);
int xeq_pbc_tables_host(int dtype, const void* cell_host, int64_t n_graphs, const int32_t reps[3], double cutoff, void* out_host,
                        int64_t out_count);
/* The same table for ONE cell that lives on the device (a box that a barostat moves: runtime.GraphedStepPBC(device_cell=True)), one
 * launch on `stream`: cell [1, 3, 3] of `dtype` in device memory, reps / pbc on the host (read at the call), out[] = grid | offs |
 * recip | thr in device memory, 6 n_cells + 12 values.  The arithmetic is the host function's own statement (csrc/xeq_pbc_tables.h)
 * in an object built without contraction: the values are the host function's bit for bit, f32 and f64.  reps_needed [3] (int32, device,
 * optional): what xeq_pbc_image_counts gives for this cell and periodicity -- a caller whose image counts are fixed (a captured graph)
 * compares. */
int xeq_pbc_tables_device(int dtype, const void* cell, const int32_t reps[3], const int32_t pbc[3], double cutoff, void* out, int64_t out_count,
                          int32_t* reps_needed, void* stream);

/* wrap_positions (data/radius_graph.py:6-32) for every atom: fractional = pos cell_inv[g], shift = floor(fractional) on the periodic
 * axes (pbc[a] != 0), pos_wrap = (fractional - shift) cell[g].  cell / cell_inv [G, 3, 3] row-major (rows = lattice vectors). */
int xeq_pbc_wrap(int dtype, const void* pos, const int64_t* ptr, int64_t n_graphs, int64_t n_nodes, const void* cell,
                 const void* cell_inv, const int32_t pbc[3], void* pos_wrap, void* shift, void* stream);
/* ------------------------------------------------------------ neighbour search */

/* ONE neighbour search in five forms, described by one argument record (the rules of the records further down: every member 8 bytes
 * wide, no padding, XEQ_REC_NEIGHBORS of xeq_record_bytes; read during the call, not retained).  `kind` names the form -- it is
 * stated, never inferred from which pointers are set -- and the form names the members it reads; a member a form needs and finds
 * NULL is refused with XEQ_ERR_INVALID_ARGUMENT and the member's name in xeq_last_error, before anything is launched.  All forms
 * emit the same canonical list: sorted by center (row 0 of edge_index), then by neighbor -- the periodic forms by
 * (neighbor * n_cells + cell) ascending -- bit for bit whichever form ran.
 *
 * XEQ_NEIGHBORS_OPEN_SWEEP   Replaces torch_cluster.radius_graph at data/transform.py:58-64 (non-PBC): same-graph pairs with
 *     d^2 < r^2 (strict), no self loops, unlimited neighbours.  One wave per center sweeps its graph.  Reads pos, ptr.
 * XEQ_NEIGHBORS_OPEN_BINS    The same list for graphs of many atoms (the sweep is O(n_g^2) per graph): per graph an axis-aligned
 *     bin grid over its bounding box, lo[G,3] / inv_w[G,3] (inverse bin width, width >= cutoff) / nbins[G,3], bin_base[G+1] =
 *     running bin count.  Count and fill visit the 3x3x3 bin block of each center with the same d^2 < r^2 arithmetic and rank
 *     the hits per center.  Reads pos, ptr, lo, inv_w, nbins, bin_base, bin_start, bin_atom.
 * XEQ_NEIGHBORS_PBC_ALL      Replaces the cdist/nonzero search of radius_graph_pbc (data/radius_graph.py:118-126, 162-181).  The
 *     caller supplies what the reference computes on the host side: wrapped positions pos[N,3] (:111), per-graph image
 *     translation vectors img[G, n_cells, 3] (:104), the integer image table cells[n_cells,3] (:97) and the per-atom wrap
 *     shift[N,3] (:113).  Pairs with 0.01 < D < cutoff, every image of every pair tested; cell_offsets = cells[cell] +
 *     shift[center] - shift[neighbor] (:186-190).  Reads pos, ptr, img, n_cells; the fill also cells, shift.
 * XEQ_NEIGHBORS_PBC_PRUNED   The same search with image pruning (default of the Python front): per (center, neighbor) pair only
 *     the image offsets n with |f_a - n_a| <= thr_a on every periodic axis are evaluated, f = (pos[c] - pos[n]) . recip^T -- a
 *     necessary condition for the pair to be within the cutoff, so the edge set and its order are those of the exhaustive form
 *     (the survivors are evaluated with the same arithmetic).  recip[G,3,3]: rows a_j x a_k / V of each cell (what
 *     data/radius_graph.py:61-82 builds for its image counts); thr[G,3] = cutoff |recip_a| + margin; reps[3] = images per axis of
 *     the enumeration (n_cells = prod (2 reps + 1), cartesian_prod order; anything else is refused).  Reads what PBC_ALL reads and
 *     recip, thr, reps.
 * XEQ_NEIGHBORS_PBC_BINS     The pruned search for graphs of many atoms.  Bins live in fractional coordinates: nbins[G,3] per axis
 *     (1 on open axes; bin width >= the cutoff across lattice planes, i.e. nbins_a <= 1 / thr_a), bin_base[G+1] = running sum of
 *     bins per graph.  Count and fill visit the 3x3x3 bin block around each center (same per-pair arithmetic and image pruning);
 *     the fill writes unordered keys and ranks them per center, which restores the reference's order.  Reads what PBC_PRUNED reads
 *     and nbins, bin_base, bin_start, bin_atom.
 *
 * The sequence: for the two bin-grid kinds first xeq_neighbors_bin_ids (keys[N] = each atom's global bin id; reads pos, ptr,
 * nbins, bin_base and lo, inv_w or recip), then the caller sorts atoms by it (xeq_csr_by_key: bin_start[n_bins + 1], bin_atom[N])
 * and sets the two members.  xeq_neighbors_count writes deg[N]; the caller scans it (xeq_exclusive_scan_i32), reads E =
 * rowptr[N] back and allocates edge_index[2, E] (periodic kinds: cell_offsets[E, 3] of `dtype`; bin-grid kinds: tmp_keys[E], NULL
 * for the others); xeq_neighbors_fill writes them.  n_nodes = 0 and (for the fill) n_edges = 0 return XEQ_OK at once.
 *
 * Capacity form (round 3): the edge count need not reach the host.  Pass a CAPACITY as n_edges of the open sweep or the pruned
 * periodic kind (edge_index [2, capacity], never written past) and hand the same capacity to the reverse-edge maps,
 * xeq_edge_vectors_fwd and the wq message entry points: every walk over the list is bounded by rowptr[n_nodes] on the device,
 * slots behind it keep whatever valid node ids they held (zero-initialise the buffer once).  This is what lets neighbour list +
 * model run as ONE captured HIP graph for batches of changing edge counts (xequinet_amd/runtime.py::GraphedStep); an
 * open-boundary list never exceeds sum_g n_g (n_g - 1). */
enum { XEQ_NEIGHBORS_OPEN_SWEEP = 0, XEQ_NEIGHBORS_OPEN_BINS = 1, XEQ_NEIGHBORS_PBC_ALL = 2, XEQ_NEIGHBORS_PBC_PRUNED = 3,
       XEQ_NEIGHBORS_PBC_BINS = 4 };

typedef struct xeq_neighbor_search {
  int64_t dtype;            /* XEQ_F32 / XEQ_F64: the type of pos, img, cells, shift, recip, thr, lo, inv_w and cell_offsets */
  int64_t kind;             /* XEQ_NEIGHBORS_* */
  int64_t n_graphs;
  int64_t n_nodes;
  int64_t n_cells;          /* periodic kinds: images in the table, > 0 */
  double cutoff;
  int64_t reps[3];          /* pruned and periodic bin-grid kinds: images per axis */
  const void* pos;          /* [N, 3]; the periodic kinds: wrapped positions */
  const int64_t* ptr;       /* [G + 1]: first atom of every graph */
  const void* img;          /* [G, n_cells, 3] */
  const void* cells;        /* [n_cells, 3] (fill) */
  const void* shift;        /* [N, 3] (fill) */
  const void* recip;        /* [G, 3, 3] */
  const void* thr;          /* [G, 3] */
  const void* lo;           /* [G, 3] */
  const void* inv_w;        /* [G, 3] */
  const int32_t* nbins;     /* [G, 3] */
  const int32_t* bin_base;  /* [G + 1] */
  const int32_t* bin_start; /* [n_bins + 1] (count, fill) */
  const int32_t* bin_atom;  /* [N] (count, fill) */
} xeq_neighbor_search;

int xeq_neighbors_bin_ids(const xeq_neighbor_search* search, int64_t* keys, void* stream);
int xeq_neighbors_count(const xeq_neighbor_search* search, int32_t* deg, void* stream);
int xeq_neighbors_fill(const xeq_neighbor_search* search, const int32_t* rowptr, int64_t n_edges, int64_t* tmp_keys, int64_t* edge_index,
                       void* cell_offsets, void* stream);

/* ------------------------------------------------------------ edge geometry */

/* Neighbour-sorted permutation of a SYMMETRIC, center-sorted edge list whose neighbours are ascending and unique
 * within a center (the open-boundary builders above emit exactly that: replaces the stable sort by neighbour that
 * ops.EdgeGraph of the reference-side caller would otherwise need, cf. torch_scatter's index_add on edge_index[1],
 * nn/xpainn.py:154-159).  rev[e] = position of the reverse edge; n_perm = rev and n_rowptr = c_rowptr.
 * rev[e] = -1 where the reverse edge is missing (the list was not symmetric). */
int xeq_reverse_edge_map(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const int32_t* c_rowptr,
                         int32_t* rev, void* stream);
/* The same for a PERIODIC list of the builders above (the XEQ_NEIGHBORS_PBC_* kinds: center-sorted, a center's edges ascending in (neighbor,
 * image)): rev[e] = position of (j <- i, -offset) for e = (i <- j, offset), -1 where the list holds no such edge.  Such a list is
 * symmetric up to a rounding at the cutoff -- the reference forms |pos_i - (pos_j + image)| (data/radius_graph.py:117-121), and the two
 * directions round differently -- so a -1 can occur for an edge within an ulp of the cutoff, where the envelope is ~1e-14 (and its
 * slope ~1e-7 of the scale): the consumers of a mirror map (XEQ_WQ_MIRROR_WALK, xeq_message_wq_edge_grad*, xeq_edge_vectors_bwd) skip
 * such an entry, the edge then misses its vanishing reverse contribution.  n_edges may be a capacity (the list ends at c_rowptr[N]).
 * With it a periodic system's reverse pass walks the forward plan like an open one's: no sort by neighbor, no second plan, no second
 * set of records (round 5; ~0.1 ms of a 1 536-atom step). */
int xeq_reverse_edge_map_pbc(int dtype, const int64_t* edge_index, const void* cell_offsets, int64_t n_edges, int64_t n_nodes,
                             const int32_t* c_rowptr, int32_t* rev, void* stream);

/* compute_edge_data (nn/basic.py:110-131): vec = pos[c] - pos[n] - cell_offsets @ cell[batch[n]],
 * dist = |vec|.  cell/cell_offsets/batch may be NULL (non-PBC).  batch == NULL with a
 * cell means single graph (cell[0], nn/basic.py:121-123). */
int xeq_edge_vectors_fwd(int dtype, const void* pos, const int64_t* edge_index, int64_t n_edges,
                         const void* cell, const void* cell_offsets, const int64_t* batch, void* vec, void* dist,
                         void* stream);

/* Backward of the above w.r.t. pos, as a deterministic segmented sum (no atomics):
 * grad_pos[i] = sum_{e: center=i} gvec[e] - sum_{e: neighbor=i} gvec[e].
 * c_rowptr/c_perm: CSR over centers (perm NULL = edges already center-sorted);
 * n_rowptr/n_perm: CSR over neighbors. */
int xeq_edge_vectors_bwd(int dtype, const void* grad_vec, int64_t n_nodes, const int32_t* c_rowptr,
                         const int32_t* c_perm, const int32_t* n_rowptr, const int32_t* n_perm, void* grad_pos,
                         void* stream);

/* --------------------------------------------- operator-level (e3nn) drop-ins */

/* e3nn.o3.SphericalHarmonics(irreps, normalize=True, "component") as built at
 * nn/xpainn.py:49-51.  `vec` is in e3nn axis order (the caller already applied
 * vec[:, [1,2,0]], nn/xpainn.py:71-74).  out[E, D], every Y_l repeated mul[l] times. */
int xeq_sph_harm_fwd(int dtype, const void* vec, int64_t n, const int32_t mul[3], int normalize, void* out,
                     void* stream);
int xeq_sph_harm_bwd(int dtype, const void* vec, const void* grad_out, int64_t n, const int32_t mul[3],
                     int normalize, void* grad_vec, void* stream);

/* SphericalBesselj0 / GaussianSmearing (nn/rbf.py:114-152) and the envelopes
 * (nn/rbf.py:43-73) on dist[E].  rbf_out[E,B], fcut_out[E] (either may be NULL). */
int xeq_radial_fwd(int dtype, const void* dist, int64_t n, int rbf_kind, int cutoff_kind, int num_basis,
                   double cutoff, const void* p0, const void* p1, void* rbf_out, void* fcut_out, void* stream);

/* e3nn.o3.ElementwiseTensorProduct(irreps, "Cx0e") (nn/xpainn.py:119-121): out[n,u,m] = x[n,u,m]*g[n,u].
 * g_rows == 1 broadcasts one gate row (EquivariantLayerNorm affine, nn/o3layer.py:164). */
int xeq_elementwise_tp_fwd(int dtype, const void* x, const void* g, int64_t n, int64_t g_rows,
                           const int32_t mul[3], void* out, void* stream);

/* TensorProduct 'uuu' l x l -> 0e with path weight ir.dim (Invariant / EquivariantDot,
 * nn/o3layer.py:23-29,89-95): out[n,u] = sum_m a[n,u,m] b[n,u,m]. */
int xeq_channel_dot_fwd(int dtype, const void* a, const void* b, int64_t n, const int32_t mul[3], void* out,
                        void* stream);
/* grad_a[n,u,m] = g[n,u] * b[n,u,m] (same kernel as the elementwise TP). */

/* EquivariantLayerNorm.forward (nn/o3layer.py:145-171) and its backward w.r.t. x. */
int xeq_eqln_fwd(int dtype, const void* x, const void* weight, const void* bias, int64_t n,
                 const int32_t mul[3], double eps, void* out, void* stream);
int xeq_eqln_bwd(int dtype, const void* x, const void* weight, const void* grad_out, int64_t n,
                 const int32_t mul[3], double eps, void* grad_x, void* stream);

/* torch_scatter.scatter_sum over a sorted index given as ptr (nn/output.py:124):
 * out[g, :] = sum_{i in [ptr[g], ptr[g+1])} src[i, :]. */
int xeq_segment_sum(int dtype, const void* src, const int64_t* ptr, int64_t n_segments, int64_t width,
                    void* out, void* stream);
/* torch_scatter.scatter(src, index, dim=0, reduce="sum") for an arbitrary index
 * (float atomics; `out` must be zero-initialised by the caller). */
int xeq_scatter_add(int dtype, const void* src, const int64_t* index, int64_t n, int64_t width, void* out,
                    int64_t n_out, void* stream);

/* The model's first message block behind XEmbedding in ONE gather (round 5): there a node's scalar features, the LayerNorm /
 * scalar_mlp output h and the 0e block of the equivariant norm are functions of the node's ELEMENT alone (nn/xpainn.py:62, 76-81,
 * 128-139: s = Linear(table[Z]), x = 0), so they are evaluated once per table row (rows_s [Zmax + 1, node_dim], rows_h [., hidden_dim],
 * rows_x0 [., node_dim]) and gathered by atomic number: s_out [n, node_dim], h_out [n, hidden_dim], xhat_out [n * irreps_dim] in BT
 * layout with every l > 0 block zero.  z: int32 or int64 atomic numbers; one outside [0, n_rows) reads row 0.  Replaces three ATen
 * gathers and a fill.  hidden_dim == 0 / irreps_dim == 0: h_out / xhat_out are not written (the table form of the wq message kernels,
 * xeq_message_fwd_wq_table below, reads the table rows themselves: only s is gathered per node). */
int xeq_first_block_front(const void* z, int z_is_int64, int64_t n, int64_t n_rows, const void* rows_s, const void* rows_h, const void* rows_x0,
                          int node_dim, int hidden_dim, int64_t irreps_dim, void* s_out, void* h_out, void* xhat_out, void* stream);

/* Up to XEQ_COPY_MANY_MAX device-to-device copies in ONE launch: dst[i][0 .. bytes[i]) = src[i][...] (whole aligned 4-byte
 * words, buffers must not overlap).  src / dst / bytes are HOST arrays.  HIP-graph replay (runtime.GraphedModel) refreshes
 * the captured inputs of an evaluation with it -- the per-step tensor hand-over the reference does with `data.to(device)`
 * (run/inference.py:39). */
/* Single f32 linear layers on the matrix cores, y = act(x W^T + b) (csrc/xeq_linear.hip): the node-side contractions that are
 * not two-layer MLPs -- dot_lin (nn/xpainn.py:191-193, :222-223) and its input gradient, the embedding Linear(56, 128) on the
 * gathered table rows (nn/xpainn.py:43-48, nn/basic.py:57: `row_index` = atomic numbers gathers the rows of x), the energy
 * head's first layer (nn/output.py:104-118).  w_packed: xeq_mlp_pack(W, b, n_out, k_in, transposed) -- transposed = 1 with
 * W given as [k_in][n_out] turns the same weight into the input-gradient product.  k_in % 8 == 0, <= 256; n_out % 32 == 0, <= 256;
 * act 0 none / 1 SiLU; pre (optional) receives the pre-activation.  A row's sums run in one fixed order whatever n is.
 * xeq_head_dot: out[n] = <hidden[n, :], w2> + b2 (the head's last layer, nn/output.py:104-106); xeq_head_bwd_hidden: its
 * reverse with the SiLU in front, g_hidden[n, j] = g_atomic[n] w2[j] silu'(pre[n, j]) (g_atomic NULL: ones). */
/* Test entry for the property the few-row forms rest on (csrc/xeq_linear_s.h): one 32 x 32 block of a [32, 224] x b [224, 32] through
 * v_mfma_f32_32x32x2_f32, through v_mfma_f32_16x16x4_f32 and as a sequential fmaf chain per element; diff[0] / diff[1] (int32, zeroed by the
 * caller) += the outputs whose bits differ between the two instruction shapes / between the matrix instruction and the chain. */
int xeq_mfma_order_probe(const float* a, const float* b, int32_t* diff, void* stream);
int xeq_linear_supported(int dtype, int k_in, int n_out);
int xeq_linear_fwd(const void* x, int64_t ldx, int64_t n, int k_in, const int32_t* row_index, const void* w_packed, int n_out,
                   int has_bias, int act, void* pre, void* y, int64_t ldy, void* stream);
int xeq_head_dot(const void* hidden, int64_t n, int hidden_dim, const void* w2, const void* b2, void* out, void* stream);
int xeq_head_bwd_hidden(const void* pre, int64_t n, int hidden_dim, const void* w2, const void* g_atomic, void* g_hidden, void* stream);
/* The whole energy head of a force evaluation in ONE launch (round 5; nn/output.py:104-128 with the reverse pass of
 * nn/basic.py:143-159): atomic[n] = <SiLU(W1 s_n + b1), w2> + b2 and, when `jac` is given, the head's reverse pass as a saved row
 * jac[n, :] = d atomic_n / d s_n = W1^T (w2 . SiLU'(W1 s_n + b1)) -- the output is one number per node, so the reverse pass of
 * whatever reaches the head is g_s[n, :] = (g_atomic[n] + g_total[batch[n]]) jac[n, :] (xeq_head_bwd; either gradient may be NULL,
 * strides in elements, 0 = a broadcast scalar; batch NULL: one graph).  w1_packed = xeq_mlp_pack(W1, b1, hidden, node_dim, 0),
 * w1t_packed = xeq_mlp_pack(W1, NULL, node_dim, hidden, 1).  Widths: multiples of 32, <= 256.  Replaces xeq_linear_fwd + xeq_head_dot
 * (+ xeq_segment_sum's reverse gather) + xeq_head_bwd_hidden + xeq_linear_fwd of the round-3 head: seven launches -> three. */
int xeq_head_supported(int dtype, int node_dim, int hidden_dim);   /* 1 / 0, not a status */
int xeq_head_fwd(const void* s, int64_t lds, int64_t n, int node_dim, int hidden_dim, const void* w1_packed, const void* w1t_packed,
                 const void* w2, const void* b2, void* atomic, void* jac, void* stream);
int xeq_head_bwd(const void* jac, int64_t n, int node_dim, const void* g_atomic, int64_t ga_stride, const void* g_total, int64_t gt_stride,
                 const int64_t* batch, void* g_s, void* stream);

/* Weight gradient of a linear layer for a TRAINING pass (what autograd forms as grad_output^T @ input for nn.Linear, utils/trainer.py:
 * 295-302; the o3.Linear blocks likewise): parts[c][M][K] = sum over the rows of chunk c of a[row, 0..M)^T b[row, 0..K), f32, rows
 * with strides lda / ldb; n_chunks = xeq_wgrad_chunks(n, M, K); dW = sum over c (fixed order: reproducible bit for bit).  with_bias:
 * every chunk's block is followed by M more floats, the column sums of a over the chunk's rows (the layer's bias gradient): parts is
 * [n_chunks][M K + M]. */
int xeq_wgrad_chunks(int64_t n, int m, int k);
int xeq_wgrad(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t n, int m, int k, int with_bias, int n_chunks, void* parts,
              void* stream);

/* A batch of n atoms in g graphs into arrays of n_cap atoms / g_cap graphs in ONE launch (runtime.GraphedStep: neighbour list +
 * model as one captured graph over capacity-sized arrays): atoms n .. n_cap - 1 get atomic number 0, positions
 * (pad0 + spacing (i - n), 0, 0) -- no two within any cutoff -- and sit alone in graph g_cap - 1; graphs g .. g_cap - 2 are empty.
 * ptr [g + 1] / ptr_out [g_cap + 1], batch [n] / batch_out [n_cap] int64; batch may be NULL: an atom's graph is then found in ptr. */
int xeq_load_padded_batch(int dtype, const void* pos, const int32_t* z, const int64_t* ptr, const int64_t* batch, int64_t n,
                          int64_t g, int64_t n_cap, int64_t g_cap, double pad0, double spacing, void* pos_out, int32_t* z_out,
                          int64_t* ptr_out, int64_t* batch_out, void* stream);
/* the same reading int64 atomic numbers (a torch.long tensor as it is: no conversion launch in front of every step) */
int xeq_load_padded_batch_z64(int dtype, const void* pos, const int64_t* z, const int64_t* ptr, const int64_t* batch, int64_t n, int64_t g,
                              int64_t n_cap, int64_t g_cap, double pad0, double spacing, void* pos_out, int32_t* z_out,
                              int64_t* ptr_out, int64_t* batch_out, void* stream);
/* a contiguous range of molecules of a larger batch (a shard of it: runtime.GraphedLanes): pos, z, batch point at the range's first
 * atom, ptr at its first graph; the range is renumbered from zero (ptr values - atom_offset, batch values - graph_offset) */
int xeq_load_padded_shard(int dtype, const void* pos, const void* z, int z_is_int64, const int64_t* ptr, const int64_t* batch, int64_t n,
                          int64_t g, int64_t atom_offset, int64_t graph_offset, int64_t n_cap, int64_t g_cap, double pad0, double spacing,
                          void* pos_out, int32_t* z_out, int64_t* ptr_out, int64_t* batch_out, void* stream);

#define XEQ_COPY_MANY_MAX 16
int xeq_copy_many(int n, const void* const* src, void* const* dst, const int64_t* bytes, void* stream);
/* The same number of buffer pairs COMPARED in one launch (runtime.GraphedModel: is the engine's neighbour list the one the captured
 * graph holds?): flag[0] = gen when any 4-byte word of any pair differs, untouched otherwise; gen: a value the flag has never held. */
int xeq_compare_many(int n, const void* const* a, const void* const* b, const int64_t* bytes, int32_t gen, int32_t* flag, void* stream);

/* ALL instructions of a general Clebsch-Gordan e3nn.o3.TensorProduct in one launch (round 4; nn/tp.py:20-107 builds the instruction lists;
 * nn/xe3net.py:133-146 'uuu' with shared weights, nn/output.py:411-421 'uuw' with one weight set per sample):
 *   out[n, off_out + w (2 l3 + 1) + k] = sum_paths coeff_p sum_{u,v} W_p[..] sum_{i,j} cg_p[i,j,k] x1[n, off1 + u (2 l1 + 1) + i] x2[n, off2 + v (2 l2 + 1) + j]
 * A workgroup stages the x1 / x2 rows of a tile of nodes and every 3j table in LDS; a thread owns an output element (a block of four w for
 * 'uvw' / 'uuw', where the bilinear form is shared by all w) and walks the paths into its block in table order: one store per element, no
 * read-modify-write, deterministic.  paths: n_paths x 10 ints (off1, off2, off_out, mul1, mul2, mul_out, l1, l2, l3, mode: 0 uvw, 1 uvu,
 * 2 uvv, 3 uuw, 4 uuu, 5 uvuv), sorted by off_out, at most 40 paths into at most 16 blocks per launch; cg: the paths' real Wigner-3j tables
 * one behind the other (device, dtype of x), cg_off[p] / cg_floats; w_off[p]: first weight of path p in `weight` (-1: unweighted), shared
 * (weight_stride 0) or per sample; coeff[p] (host).  The reverse passes w.r.t. x1 / x2 are the same entry on (grad_out, x2) / (x1, grad_out)
 * with permuted tables and the connection mode of the transposed contraction (xequinet_amd/tp.py::_REVERSE).
 * xeq_tensor_product_wgrad: dL/dW of the weighted paths (same table; w_off increasing, w_numel[p] weights per path): shared = 1 writes
 * parts [xeq_tensor_product_wgrad_chunks(n), w_total] (the caller adds the chunks in order), shared = 0 writes dW [n, w_total].
 * xeq_tensor_product_form: the form xeq_tensor_product takes for a pass (no launch, no GPU needed): -1 the tied form (every path 'uuu' /
 * 'uuw' / 'uvu' / 'uvv': a wave per node, a lane per channel), t > 0 the tile form on t nodes per workgroup, 0 when not one row of x1 | x2
 * fits the LDS tile behind the 3j tables -- xeq_tensor_product refuses such a pass, the caller launches xeq_tensor_product_path per path. */
int xeq_tensor_product(int dtype, const void* x1, const void* x2, int64_t n, int dim1, int dim2, int dim_out, int n_paths,
                       const int32_t* paths, const void* cg, const int32_t* cg_off, int cg_floats, const void* weight, int64_t weight_stride,
                       const int32_t* w_off, const double* coeff, void* out, void* stream);
int xeq_tensor_product_form(int dtype, int64_t n, int dim1, int dim2, int n_paths, const int32_t* paths, int cg_floats);
int64_t xeq_tensor_product_wgrad_chunks(int64_t n);
int xeq_tensor_product_wgrad(int dtype, const void* x1, const void* x2, const void* g, int64_t n, int dim1, int dim2, int dim_out, int n_paths,
                             const int32_t* paths, const void* cg, const int32_t* cg_off, const int32_t* w_off, const int32_t* w_numel, int w_total,
                             const double* coeff, int shared, void* parts, void* stream);

/* One instruction of a general Clebsch-Gordan e3nn.o3.TensorProduct (nn/tp.py:20-107 builds the instruction lists;
 * nn/xe3net.py:133-146 'uuu', nn/output.py:411-421 'uuw'):
 *   out[n, off_out + w (2 l3 + 1) + k] += coeff * sum_{u,v} W[..] sum_{i,j} cg[i,j,k] x1[n, off1 + u (2 l1 + 1) + i] x2[n, off2 + v (2 l2 + 1) + j]
 * mode: 0 uvw, 1 uvu, 2 uvv, 3 uuw, 4 uuu, 5 uvuv (e3nn connection modes: which of u, v, w are tied); cg = the real
 * Wigner-3j table [2 l1 + 1, 2 l2 + 1, 2 l3 + 1] (device memory, dtype of x); weight NULL = unweighted path, otherwise
 * the path's weights in e3nn's order, shared (weight_stride 0) or one set per sample (weight_stride = floats per sample).
 * The launches of a product's paths accumulate into a zero-initialised `out` in stream order: deterministic. */
int xeq_tensor_product_path(int dtype, const void* x1, const void* x2, int64_t n, int dim1, int dim2, int dim_out, int off1,
                            int off2, int off_out, int mul1, int mul2, int mul_out, int l1, int l2, int l3, int mode,
                            const void* cg, const void* weight, int64_t weight_stride, double coeff, void* out, void* stream);

/* ------------------------------------------------------------ fused message */

/* GENERIC form (64-bit offsets, f32 / f64, up to 256 channels per kind): the fallback for sizes and layouts the
 * _wq and _sb forms below do not take.
 * XPainnMessage.forward lines nn/xpainn.py:140-159 in one pass over
 * destination-sorted edges (K5-K7, K11-K16 of SURVEY 2.2):
 *   filter = (rbf(d) W^T + b) * fcut(d)                       :140
 *   g = h[nbr] * filter = [gate_state C | gate_edge C | msg_s F]  :142-148
 *   msg_x = xhat[nbr] (x) gate_state + Y(vec) (x) gate_edge    :150-154
 *   s_out = s_in + sum_{e->c} msg_s ; x_out = x_in + sum msg_x  :158-159
 * rbf / fcut / Y_lm are recomputed from vec per edge and never materialised.
 * h[N, 2C+F] = scalar_mlp output (:139), xhat[N, D] = o3norm output (:131).
 * rowptr[N+1]/perm[E]: CSR over centers (perm NULL = already sorted);
 * nbr = edge_index row 1 (int64[E]); vec[E,3] in ORIGINAL axis order.
 * Per-node segmented sum in registers: no atomics, bitwise reproducible. */
int xeq_message_fwd(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* perm,
                    const int64_t* nbr, const void* vec, const void* h, const void* xhat, const void* s_in,
                    const void* x_in, const void* w_rbf, const void* b_rbf, const void* p0, const void* p1,
                    int rbf_kind, int cutoff_kind, int num_basis, double cutoff, int node_dim,
                    const int32_t mul[3], void* s_out, void* x_out, int xhat_layout, void* stream);

/* Reverse pass of the fused message w.r.t. h, xhat and vec (what the force
 * evaluation nn/basic.py:143-159 needs; parameter gradients are out of scope).
 * Iterates the CSR over NEIGHBORS (n_rowptr/n_perm; n_perm NULL = edges sorted by
 * neighbor) so grad_h / grad_xhat are segmented sums too; grad_vec[E,3] is written
 * at the edge's own position.  center = edge_index row 0. */
int xeq_message_bwd(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm,
                    const int64_t* center, const void* vec, const void* h, const void* xhat, const void* grad_s,
                    const void* grad_x, const void* w_rbf, const void* b_rbf, const void* p0, const void* p1,
                    int rbf_kind, int cutoff_kind, int num_basis, double cutoff, int node_dim,
                    const int32_t mul[3], void* grad_h, void* grad_xhat, void* grad_vec, int xhat_layout,
                    void* stream);

/* Parameter gradients of the radial filter for a TRAINING pass (rbf_lin.weight / .bias, nn/xpainn.py:117,140; the trainable
 * basis parameters freq, nn/rbf.py:143-146, or mean / std, :121-125) -- what autograd gets in the reference by differentiating
 * through the materialised filter[E, 576] (nn/basic.py:154-155 with create_graph=training, utils/trainer.py:295-302).  Same walk
 * and operands as xeq_message_bwd (neighbor-sorted CSR, center = edge_index row 0, grad_s / grad_x = dL/ds_out, dL/dx_out);
 * writes parts[n_parts][H][3 B + 1] (n_parts = xeq_message_param_grad_parts(n_nodes)), per filter row c:
 *   [0, B)        sum_e G f rho_k             -> dL/dW[c, k] after the sum over parts
 *   [B]           sum_e G f                   -> dL/db[c]
 *   [B+1, 2B+1)   sum_e G f d rho_k / d p0_k  -> dL/dp0_k = sum_c W[c, k] (.)
 *   [2B+1, 3B+1)  sum_e G f d rho_k / d p1_k  -> dL/dp1_k likewise (zeros for the Bessel basis)
 * with G[e, c] = dL/dfilter_out[e, c] h[nbr(e), c].  f32 and f64; node_dim and the channel count at most 256 each. */
int xeq_message_param_grad_parts(int64_t n_nodes);
int xeq_message_param_grad(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm,
                           const int64_t* center, const void* vec, const void* h, const void* xhat, const void* grad_s,
                           const void* grad_x, const void* p0, const void* p1, int rbf_kind, int cutoff_kind, int num_basis,
                           double cutoff, int node_dim, const int32_t mul[3], int xhat_layout, int n_parts, void* parts,
                           void* stream);

/* The same parameter gradients on the matrix cores (csrc/xeq_train.hip; f32, node_dim and multiplicities in multiples of 32, a table
 * row of 64 floats: xeq_message_param_grad_mc_supported).  xeq_param_basis writes, once per training step, the per-edge rows
 *   tab[e][W] = f(d_e) [rho_k (B) | 1 | d rho_k/d p0 (B) | d rho_k/d p1 (B, gaussian basis only)], zero padding to a multiple of 4, Y_1 (3), Y_2 (5)
 * (W = xeq_param_basis_width: whole 128-byte lines) in the order of the edge list; xeq_message_param_grad_mc contracts them with G[e, c] formed on the fly:
 * parts[n_parts][H][64], columns as xeq_message_param_grad's (the caller sums over the parts).  center / nbr = edge_index rows 0 / 1;
 * any edge order (center-sorted lists gather best).  n_valid (optional, device pointer): the edge count of a capacity-sized list whose
 * size never reached the host (a training step captured as one HIP graph, train.GraphedTrainStep): edges behind it are not walked. */
int xeq_message_param_grad_mc_supported(int dtype, int rbf_kind, int num_basis, int node_dim, const int32_t mul[3]);
int xeq_param_basis_width(int rbf_kind, int num_basis);
int xeq_message_param_grad_mc_parts(int64_t n_edges, int node_dim, const int32_t mul[3]);
int xeq_param_basis(const void* vec, int64_t n_edges, int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0,
                    const void* p1, void* tab, void* stream);
int xeq_message_param_grad_mc(int64_t n_nodes, int64_t n_edges, const int64_t* center, const int64_t* nbr, const void* tab, const void* h,
                              const void* xhat, const void* grad_s, const void* grad_x, int rbf_kind, int num_basis, int node_dim,
                              const int32_t mul[3], int xhat_layout, int grad_x_layout, const int32_t* n_valid, int n_parts, void* parts,
                              void* stream);
/* Affine-parameter gradients of a block's two norms for a TRAINING pass (nn.LayerNorm weight / bias on the scalars,
 * EquivariantLayerNorm affine_weight / affine_bias, nn/o3layer.py:145-171), f32: from the block inputs s [n, F], x [n, D], the
 * statistics stats [n, 4] the forward norm kernel wrote, dL/dshat rows (stride ld_gs) and dL/dxhat in the BT layout.
 * parts[n_chunks][2 F + C + mul0] = [d ln_w | d ln_b | d eq_w | d eq_b] per row chunk (n_chunks = xeq_norm_param_grad_chunks(n));
 * the caller sums the chunks (fixed order). */
int xeq_norm_param_grad_chunks(int64_t n_nodes);
int xeq_norm_param_grad(const void* s, const void* x, const void* stats, const void* g_shat, int64_t ld_gs, const void* g_xhat_bt,
                        int64_t n_nodes, int node_dim, const int32_t mul[3], int n_chunks, void* parts, void* stream);
/* f32 x[n_nodes, D] in the e3nn mul_ir layout -> the internal BT layout (per l a row-major [N (2l+1), mul_l] matrix; layout 1 of the
 * xhat_layout / grad_x_layout arguments): the gradient kernel's gathers of dL/dx_out rows are contiguous over the channels there. */
int xeq_to_bt(const void* x, int64_t n_nodes, const int32_t mul[3], void* out, void* stream);

/* Node-side functions of a training pass that is differentiated TWICE (forces in the loss: nn/basic.py:143-159 with create_graph=training,
 * utils/trainer.py:295-308; host side ops.NormFn / UvFn / UpdateOutFn, csrc/xeq_train_node.hip).  f32 / f64.  Every entry has a forward
 * form (reverse = 0) and a reverse form (reverse = 1); with the *_tan pointers given, the same body runs on dual numbers (value, tangent)
 * and the outputs are the TANGENTS -- that is the second order: for the cotangent u of a first-order input gradient, the forward form at
 * tangent u gives d<u, xbar>/dg, the reverse form at tangent u gives d<u, xbar>/dx and d<u, xbar>/dtheta.
 *
 * xeq_train_norm: (s[N, F], x[N, D]) -> (LayerNorm(s), EquivariantLayerNorm(x))  (nn/xpainn.py:130-131, :213-214; nn/o3layer.py:145-171:
 *   the l = 0 block is centred, one rms over all C channels, weight per channel, bias on the l = 0 block).  xhat_layout 0: the e3nn row,
 *   1: BT (per l a row-major [N (2l+1), mul_l] matrix, one after the other) -- of out_x (forward) and of g_x (reverse).
 *   reverse: out_s / out_x = dL/ds, dL/dx (e3nn rows); rows[N, 2F + C + mul0] = per-node [d ln_w | d ln_b | d eq_w | d eq_b] (the caller sums).
 * xeq_train_uv: uv[l] = [N (2l+1), 2 mul_l] row-major (U | V of update_U / update_V in BT rows) -> out[N, 2C] = [Invariant(V) | sum_m U V]
 *   (nn/o3layer.py:40-44, :61-68; eps of the Invariant).  reverse: g = dL/dout, d_uv[l] = dL/duv[l].
 * xeq_train_out: (uv, a[N, C + 2F] = [a_vv | a_sv | a_ss], inner[N, F]) -> out0[N, F] = a_sv inner + a_ss, out1[N, D] = U a_vv (e3nn row)
 *   (nn/xpainn.py:226-230 without the residual).  reverse: g_s, g_x = dL/dout0, dL/dout1; out0 = dL/da, out1 = dL/dinner, d_uv.
 * N == 0: every entry returns XEQ_OK without a launch once the sizes (and the layout) are accepted, whatever the pointers are -- the
 *   tensors of an empty batch have null pointers. */
int xeq_train_norm(int dtype, int reverse, int64_t n, const void* s, const void* s_tan, const void* x, const void* x_tan, const void* ln_w,
                   const void* ln_b, const void* eq_w, const void* eq_b, const void* g_s, const void* g_x, int node_dim,
                   const int32_t mul[3], double eps_ln, double eps_eq, int xhat_layout, void* out_s, void* out_x, void* rows, void* stream);
int xeq_train_uv(int dtype, int reverse, int64_t n, const void* const uv[3], const void* const uv_tan[3], const void* g, const int32_t mul[3],
                 double eps, void* out, void* const d_uv[3], void* stream);
int xeq_train_out(int dtype, int reverse, int64_t n, const void* const uv[3], const void* const uv_tan[3], const void* a, const void* a_tan,
                  const void* inner, const void* inner_tan, const void* g_s, const void* g_x, int node_dim, const int32_t mul[3],
                  void* out0, void* out1, void* const d_uv[3], void* stream);

/* Edge geometry of an evaluation that is differentiated twice with respect to the POSITIONS (hessian.py; csrc/xeq_train_edge.hip, host
 * side nn/training_ops.py EdgeRecordFn / EdgeRecordGrad): vec[E, 3] -> the per-edge record [E, W], W = xeq_edge_basis_width(B), in
 * xeq_edge_basis's layout [f rho_k (B) | 0 to a multiple of 4 | f | Y_1 (3) | Y_2 (5) | 0 0 0], with the values of the tensor chain of
 * nn/training.py (component-normalised harmonics in (y, z, x) order, norm clamped at 1e-12; f and all its derivatives 0 at |vec| >= cutoff).
 * Dual-number convention of xeq_train_norm: with a *_tan pointer given the same body runs on (value, tangent) and `out` holds the TANGENT.
 *   reverse = 0: out[E, W] = record(vec); with vec_tan: J(vec) vec_tan.  g_rec / g_rec_tan must be NULL.
 *   reverse = 1: out[E, 3] = dL/dvec = J(vec)^T g_rec; with tangents: the tangent of that at (vec + eps vec_tan, g_rec + eps g_rec_tan);
 *                either tangent may be NULL (= zero).
 * Pad columns and the last three entries of a record are written as exact zeros.  p0 / p1: the basis parameters (Bessel: freq; Gaussian:
 * mean, std), inputs only -- no parameter gradient.  f32 / f64, Bessel and Gaussian bases, both envelopes, num_basis 1..32;
 * xeq_train_edge_supported -> 1 / 0 says so (0 for the exponential bases, which the entry refuses).  n_edges = 0: success, no launch. */
int xeq_train_edge_supported(int dtype, int rbf_kind, int cutoff_kind, int num_basis);
int xeq_train_edge(int dtype, int reverse, int64_t n_edges, const void* vec, const void* vec_tan, const void* g_rec, const void* g_rec_tan,
                   int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1, void* out, void* stream);

/* Launch policy, stated ONCE for every front (the Python modules' ops.select_message_impl / ops._wq_edges_per_stream and the
 * registered operator xeq::xpainn_eval call these): the kernel family `auto` takes for a configuration and these sizes, and the
 * stream length of a wq walk plan (n_ranges = ceil(E / (2 x edges_per_stream))). */
#define XEQ_FAMILY_WQ 0
#define XEQ_FAMILY_SB 1
#define XEQ_FAMILY_GENERIC 3
int xeq_message_auto_family(int dtype, int64_t n_nodes, int64_t n_edges, int num_basis, int node_dim, const int32_t mul[3]);
int xeq_message_wq_edges_per_stream(int64_t n_nodes, int64_t n_edges);

/* "Scalar broadcast" form of the fused message (default path, f32 and f64).  The per-edge quantities
 * every channel shares -- f*rho_k(d), f, Y_lm, and their d/dd companions -- are evaluated once per
 * model evaluation into 4*(roundup(B,4)+12)-byte records (xeq_edge_basis), shared by all message
 * blocks and both directions; the message kernels fetch them with scalar loads (the edge index is
 * workgroup-uniform) and need no LDS and no barriers in the forward pass.
 * basis[E, W] / dbasis[E, W], W = xeq_edge_basis_width(B); dbasis may be NULL when only the forward
 * pass is needed.  Same semantics as xeq_message_fwd / xeq_message_bwd otherwise; s_in / x_in of xeq_message_fwd_sb may be NULL
 * (the aggregate without the residual: what the training pass's ops.DiffMessage asks for). */
int xeq_edge_basis_width(int num_basis);
/* 1 / 0: at most 256 channels per kind, num_basis <= 32, 32-bit element offsets (n_nodes max(H, D) < 2^31) */
int xeq_message_sb_fits(int64_t n_nodes, int64_t n_edges, int num_basis, int node_dim, const int32_t mul[3]);
int xeq_edge_basis(int dtype, const void* vec, int64_t n_edges, int rbf_kind, int cutoff_kind, int num_basis,
                   double cutoff, const void* p0, const void* p1, void* basis, void* dbasis, void* stream);
int xeq_message_fwd_sb(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* perm,
                       const int64_t* nbr, const void* basis, const void* h, const void* xhat, const void* s_in,
                       const void* x_in, const void* w_rbf, const void* b_rbf, int num_basis, int node_dim,
                       const int32_t mul[3], void* s_out, void* x_out, int xhat_layout, void* stream);
int xeq_message_bwd_sb(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm,
                       const int64_t* center, const void* basis, const void* dbasis, const void* h, const void* xhat,
                       const void* grad_s, const void* grad_x, const void* w_rbf, const void* b_rbf, int num_basis,
                       int node_dim, const int32_t mul[3], void* grad_h, void* grad_xhat, void* grad_vec,
                       int xhat_layout, void* stream);

/* The reverse pass in the form a TRAINING pass differentiates a second time (force loss: nn/basic.py:143-159 with create_graph=training,
 * utils/trainer.py:295-308; host side ops.DiffMessage).  The message nn/xpainn.py:140-159 is multilinear in (dL/dout, h, xhat | Y, the
 * record head f rho_k | f, the rbf_lin rows), so each second-order term is xeq_message_fwd_sb or this entry with ONE operand replaced by
 * its tangent.  Records as xeq_edge_basis writes them (here formed by the caller, differentiably).  Walk and operands of xeq_message_bwd_sb;
 * instead of dL/dvec it writes
 *   q[E, 2C+F]  = h[nbr(e), c] P[e, c]   (P = <dL/dx_out[center], xhat[nbr]>, <dL/dx_out[center], Y_e>, dL/ds_out[center]) -- the caller gets
 *                 dL/d(record head) = q [W | b] and dL/d[W | b] = q^T (record head) from two library GEMMs;
 *   gy[E, 8]    = dL/dY_1[3], dL/dY_2[5] of the edge.
 * flags: bit 0 the xhat layout, XEQ_SB_Y0_ZERO (also accepted by xeq_message_fwd_sb's xhat_layout): the l = 0 harmonic counts as 0 -- the
 * record holds a tangent of the harmonics; XEQ_SB_Q_ACCUMULATE: q += instead of q =; XEQ_SB_NO_GY.  f32 / f64. */
#define XEQ_SB_Y0_ZERO 8
/* xeq_message_bwd_sb only: xhat_layout | XEQ_SB_ACCUM_VEC ADDS dL/dvec to what grad_vec holds instead of storing it: the message blocks of
 * one force evaluation share one buffer (the last block of the model stores, the earlier ones add -- the order in which autograd would
 * sum their separate results, without its two elementwise launches per evaluation). */
#define XEQ_SB_ACCUM_VEC 16
#define XEQ_SB_Q_ACCUMULATE 16
#define XEQ_SB_NO_GY 32   /* gy is not wanted (and not written) */
int xeq_message_bwd_sbq(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm,
                        const int64_t* center, const void* basis, const void* h, const void* xhat, const void* grad_s,
                        const void* grad_x, const void* w_rbf, const void* b_rbf, int num_basis, int node_dim,
                        const int32_t mul[3], void* grad_h, void* grad_xhat, void* q, void* gy, int flags, void* stream);
/* dL/d[W | b] from those products: parts[n_chunks][2C+F][roundup(B, 4) + 1] with out[c, k] = sum_e q[e, c] basis[e, k] over the chunk's
 * edges (columns [0, B): dL/dW[c, k]; column roundup(B, 4): dL/db[c]); the caller adds the chunks in order.  At most 768 filter rows. */
/* Two of the three second-order passes in one walk each: pass A (h <- u_h) and pass B ((xhat, Y) <- (u_xhat, u_Y); the l = 0 harmonic counts as
 * 0, the scalar message has no term) use the TRUE record head, i.e. the same filter values and the same gathered rows; the pair kernels
 * evaluate the filter once per edge.  basis_u: records whose harmonics are u_Y (only their tail is read).
 *   xeq_message_fwd_sb_pair:  s_out = s_in + A's scalar aggregate, x_out = x_in + A's + B's equivariant aggregates (s_in / x_in may be NULL);
 *   xeq_message_bwd_sbq_pair: grad_h = B's dL/dh, grad_xhat = A's dL/dxhat, q = q_A + q_B, gy = A's dL/dY. */
int xeq_message_fwd_sb_pair(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* perm, const int64_t* nbr,
                            const void* basis, const void* basis_u, const void* h, const void* u_h, const void* xhat, const void* u_xhat,
                            const void* s_in, const void* x_in, const void* w_rbf, const void* b_rbf, int num_basis, int node_dim,
                            const int32_t mul[3], void* s_out, void* x_out, int xhat_layout, void* stream);
int xeq_message_bwd_sbq_pair(int dtype, int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm,
                             const int64_t* center, const void* basis, const void* basis_u, const void* h, const void* u_h, const void* xhat,
                             const void* u_xhat, const void* grad_s, const void* grad_x, const void* w_rbf, const void* b_rbf, int num_basis,
                             int node_dim, const int32_t mul[3], void* grad_h, void* grad_xhat, void* q, void* gy, int flags, void* stream);
/* Rows [*n_valid, n_rows) of a row-major buffer of 4-byte words := 0 (n_valid: device pointer).  For q and a capacity-sized edge list whose
 * true count never reached the host (train.GraphedTrainStep): xeq_message_bwd_sbq writes the rows of walked edges only, the two products
 * above read every row. */
int xeq_zero_rows_from(void* buf, int64_t row_words, int64_t n_rows, const int32_t* n_valid, void* stream);
int xeq_message_q_wgrad_chunks(int64_t n_edges);
int xeq_message_q_wgrad(int dtype, const void* q, const void* basis, int64_t n_edges, int num_basis, int node_dim, const int32_t mul[3],
                        int n_chunks, void* parts, void* stream);

/* "Wave / quad" form of the fused message (f32; the default whenever the channel layout allows it: node_dim == mul[0], mul[l] % 32 == 0,
 * num_basis <= 31).  The filter (rbf_lin, nn/xpainn.py:117,140: [2C+F, B+1] x [B+1] per edge) runs on the matrix cores with the channel
 * on the lane (the first sixteen basis functions as split-bf16 products, the rest and the bias column as exact-f32 steps); each half-wave
 * is a STREAM over a contiguous range of CSR segments, so the aggregation (index_add, nn/xpainn.py:158-159) is a running sum in registers
 * that is stored once per node: deterministic, no atomics, no read-modify-write (nn/xpainn.py:140-159 and its reverse pass), on a
 * PADDED walk order: every node's edge list is padded to a multiple of four slots (a "quad" = the four accumulator
 * registers 4g..4g+3 of a lane; padding slots carry an all-zero record), so a quad belongs to one node and the segment
 * logic (reset / residual / the node's only store) runs once per quad instead of once per row.
 *   xeq_message_wq_plan: the walk plan of one direction, from the CSR of the walk order (rowptr[N+1], perm[E] = edge id
 *     per slot or NULL), owner / gather = the edge_index rows the walk is sorted by / gathers from (forward: center /
 *     neighbor; reverse: neighbor / center).  Outputs, sized for P = xeq_message_wq_pcap(N, E) padded slots:
 *     qptr[N+1] (first quad per node), pgath[P] (gathered node per padded slot), peid[P] (edge id, -1 for pads),
 *     qinfo[P/4] (owner | first << 30 | last << 31 per quad), sq / sn[2 n_ranges + 1] (quad / node boundaries of the
 *     streams, on segment starts at about equal quad counts), win[xeq_message_wq_win_ints(n_ranges)] (per STEP = xeq_message_wq_waves()
 *     consecutive ranges, walked together by the waves of a workgroup: first gathered node and row count of the window that
 *     holds every node the step gathers from; since round 6 for two stream CLASSES -- the table's streams, walked by the l > 0
 *     units, and for large batches streams of three table streams each, walked by the l = 0 units -- one table behind the
 *     other).  workspace: xeq_message_wq_plan_workspace(N) bytes.
 *     Depends on the graph only, not on the positions.
 *   xeq_edge_basis_wq: per-edge records IN PADDED WALK ORDER, basis / dbasis [P, xeq_message_wq_record_floats_for(num_basis)] floats
 *     ([12 even k | 12 odd k | Y1[3] Y2[5]], value and d/dd; dbasis may be NULL), once per evaluation and direction.
 *   xeq_message_fwd_wq / _bwd_wq: one launch per message block and direction.  A workgroup walks a chunk of steps; per step it stages the window's
 *     rows (the unit's columns of h and xhat, or of grad_x and grad_s) in LDS with 16-byte loads when they fit 48 KB --
 *     batches of molecules: a few molecules -- and the per-row gathers become LDS reads; a step whose window does not fit
 *     (periodic systems, large graphs) gathers from global memory. rowptr is the CSR of the walk order (nodes without edges keep
 *     s_in / x_in, or get zero gradients).  parts[xeq_message_wq_parts_floats(N, E, mul)]: per-unit partials of dL/dd
 *     and dL/dY_lm by padded slot of the reverse walk; xeq_message_wq_edge_grad sums them in fixed unit order into
 *     grad_vec[E,3] at the edge's own position. */
int xeq_message_wq_supported(int num_basis, int node_dim, const int32_t mul[3]);   /* 1 / 0, not a status */
int xeq_message_wq_fits(int64_t n_nodes, int64_t n_edges, int num_basis, int node_dim, const int32_t mul[3]);   /* 1 / 0 */
int64_t xeq_message_wq_pcap(int64_t n_nodes, int64_t n_edges);                      /* a size, not a status */
int xeq_message_wq_waves(void);
int xeq_message_wq_record_floats_for(int num_basis);   /* floats per padded slot of a record buffer: 40 up to 23 basis functions, 48 up to 31 */
int xeq_message_wq_record_floats(void);   /* floats per padded slot of a record buffer (basis / dbasis of xeq_edge_basis_wq) */   /* ranges per step (= waves per workgroup): win holds 2 ceil(n_ranges / that) entries */
int64_t xeq_message_wq_plan_workspace(int64_t n_nodes);                             /* bytes, -1 on failure */
int64_t xeq_message_wq_win_ints(int n_ranges);                                      /* ints of a plan's window table `win` (a size, not a status) */
int xeq_message_wq_plan(const int32_t* rowptr, const int32_t* perm, const int64_t* owner, const int64_t* gather,
                        int64_t n_nodes, int64_t n_edges, int n_ranges, void* workspace, int64_t workspace_bytes,
                        int32_t* qptr, int32_t* pgath, int32_t* peid, int32_t* qinfo, int32_t* sq, int32_t* sn, int32_t* win,
                        void* stream);
int xeq_edge_basis_wq(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                      int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1,
                      void* basis, void* dbasis, void* stream);
int xeq_message_fwd_wq(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                       const int32_t* c_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis, const void* h,
                       const void* xhat, const void* s_in, const void* x_in, const void* w_rbf, const void* b_rbf,
                       int num_basis, int node_dim, const int32_t mul[3], void* s_out, void* x_out, int xhat_layout,
                       void* stream);
int64_t xeq_message_wq_parts_floats(int64_t n_nodes, int64_t n_edges, const int32_t mul[3]);   /* a size, not a status */
/* grad_h / grad_xhat may both be NULL: only the per-edge partials (dL/dvec) are formed.
 * xhat_layout of the _wq entries carries an optional hint: xhat_layout | XEQ_XHAT_HIGHER_L_ZERO promises that xhat is zero on
 * every l > 0 column.  That is the model's first message block (XEmbedding hands over x = 0, nn/xpainn.py:76-81, and the
 * equivariant layer norm of zero is zero off the 0e columns): the forward kernel then drops the gate_state term of the l > 0
 * units with its filter and gathers (bit-identical results), the reverse kernel (with grad_h NULL) drops the value filters
 * and pass S of the l > 0 units.  The other kernel families accept the hint and ignore it. */
#define XEQ_XHAT_HIGHER_L_ZERO 2
/* xeq_message_bwd_wq only: xhat_layout | XEQ_WQ_MIRROR_WALK walks the FORWARD plan (center-sorted CSR, owner = center, gathered =
 * neighbor) and its records: every slot (i <- j) then stands for its mirror edge (j <- i), whose neighbor is the owner and whose
 * center is the gathered node -- the edges a reverse walk visits for node i, in the same order, when the list is symmetric with
 * neighbours ascending per center (what the open-boundary builders of this library write).  The mirror's vector is the negative of
 * the slot's: same distance, same Y_2, Y_1 negated (done at the load), so the results are the reverse plan's bit for bit, and the
 * reverse plan and its records are never built.  xeq_message_wq_edge_grad then takes `mirror` = the reverse-edge map
 * (xeq_reverse_edge_map: position of edge (j, i) for edge (i, j)) to write each slot's gradient to the mirror edge; NULL otherwise. */
#define XEQ_WQ_MIRROR_WALK 4
/* xeq_message_fwd_wq / _bwd_wq: xhat_layout | XEQ_WQ_PACKED_WEIGHTS says that `w_rbf` points at the output of
 * xeq_message_wq_pack_weights (the units' rbf_lin rows -- bf16 splits of the first sixteen basis columns, the exact-f32 tail and the
 * bias -- in the kernels' LDS layout, xeq_message_wq_packed_weight_floats floats, once per weight version) and `b_rbf` is ignored: the
 * workgroups then stage their unit's weights with coalesced 16-byte loads instead of one row per lane (~11 us per launch). */
#define XEQ_WQ_PACKED_WEIGHTS 64
int64_t xeq_message_wq_packed_weight_floats(int num_basis, int node_dim, const int32_t mul[3]);   /* a size (-1: unsupported), not a status */
int xeq_message_wq_pack_weights(const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* packed,
                                void* stream);
int xeq_message_bwd_wq(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                       const int32_t* n_rowptr, const int32_t* pgath, const int32_t* qinfo, const void* basis,
                       const void* dbasis, const void* h, const void* xhat, const void* grad_s, const void* grad_x,
                       const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* grad_h,
                       void* grad_xhat, void* parts, int xhat_layout, void* stream);
/* TABLE FORM of the model's first message block.  Behind XEmbedding a node's h = scalar_mlp(norm(s)) and the 0e block of its xhat are
 * functions of its element alone: rows of the element table that xeq_first_block_front gathers from (h_table [T, H], xhat0_table
 * [T, F]; row = atomic number, a number outside the table reads row 0).  The _table entries read those rows instead of the per-node
 * copies, with the results of xeq_message_fwd_wq / _bwd_wq under XEQ_XHAT_HIGHER_L_ZERO bit for bit:
 *   xeq_edge_basis_wq_table: xeq_edge_basis_wq, whose launch also writes the table rows the message kernels index by -- slot_rows[P]:
 *     row of the node every padded slot gathers from; quad_rows[P / 4]: row of every quad's owner (pgath, qinfo: the plan's; z: the
 *     atomic numbers [N], int32 or int64).  Sequential loads next to the plan's arrays: no load through the node id inside a tile.
 *   xeq_message_fwd_wq_table: every workgroup copies its unit's columns of the whole table into LDS once; a gathered row is an LDS read
 *     at the slot's table row: no window, no staging and no barrier per step.  slot_rows takes pgath's place.
 *   xeq_message_bwd_wq_table: the first block of a force evaluation (no node gradients: only `parts`); the owners' rows are read from the
 *     table -- the few cache-resident rows of the species present -- at quad_rows; the gradient window is per node and stays.
 * xhat_layout: 1 | XEQ_XHAT_HIGHER_L_ZERO (| XEQ_WQ_MIRROR_WALK | XEQ_WQ_PACKED_WEIGHTS).  T <= xeq_message_wq_table_max_rows().
 * xeq_message_wq_first_table (host only; 1 / 0) is the ONE statement of when a front takes these entries: the block runs the wq family
 * (family == XEQ_FAMILY_WQ), its front half comes from the element table with T rows that fit (1 <= T <= max_rows; not behind a charge /
 * spin embedding: per_node_front), nothing wants parameter gradients (training), and XEQ_WQ_FIRST_TABLE is not "0". */
int xeq_message_wq_table_max_rows(void);
int xeq_message_wq_first_table(int family, int64_t table_rows, int training, int per_node_front);
int xeq_edge_basis_wq_table(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                            int rbf_kind, int cutoff_kind, int num_basis, double cutoff, const void* p0, const void* p1,
                            void* basis, void* dbasis, const int32_t* pgath, const int32_t* qinfo, const void* z, int z_is_int64,
                            int64_t table_rows, int32_t* slot_rows, int32_t* quad_rows, void* stream);
int xeq_message_fwd_wq_table(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                             const int32_t* c_rowptr, const int32_t* slot_rows, const int32_t* qinfo, const void* basis,
                             const void* h_table, const void* xhat0_table, int64_t table_rows, const void* s_in, const void* x_in,
                             const void* w_rbf, const void* b_rbf, int num_basis, int node_dim, const int32_t mul[3], void* s_out,
                             void* x_out, int xhat_layout, void* stream);
int xeq_message_bwd_wq_table(int64_t n_nodes, int64_t n_edges, int n_ranges, const int32_t* sq, const int32_t* sn, const int32_t* win,
                             const int32_t* n_rowptr, const int32_t* pgath, const int32_t* qinfo, const int32_t* quad_rows,
                             const void* basis, const void* dbasis, const void* h_table, const void* xhat0_table, int64_t table_rows,
                             const void* grad_s, const void* grad_x, const void* w_rbf, const void* b_rbf, int num_basis, int node_dim,
                             const int32_t mul[3], void* parts, int xhat_layout, void* stream);
int xeq_message_wq_edge_grad(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                             const int32_t* mirror, const int32_t mul[3], const void* parts, void* grad_vec, void* stream);
/* The same for the partials of SEVERAL message blocks of one evaluation (all walked on the same plan): parts[0 .. n_sets) are summed
 * per quantity in that order before the chain rule runs once (it is linear in dL/dd, dL/dY_lm): the three blocks' contributions to
 * dL/dvec -- which autograd otherwise adds up with elementwise launches behind three edge-gradient launches, nn/basic.py:143-159 over
 * nn/xpainn.py:140-159 -- in ONE launch.  n_sets <= XEQ_WQ_MAX_PART_SETS; `parts` is a HOST array of device pointers. */
#define XEQ_WQ_MAX_PART_SETS 8
int xeq_message_wq_edge_grad_sum(const void* vec, int64_t n_nodes, int64_t n_edges, const int32_t* qptr, const int32_t* peid,
                                 const int32_t* mirror, const int32_t mul[3], int n_sets, const void* const* parts, void* grad_vec,
                                 void* stream);

/* ------------------------------------------------- node-side fused elementwise stages
 * Internal "BT" layout of equivariant intermediates (xhat_layout = 1 above): block-major over
 * l, then node, then m, then channel: addr(n, u' in block l, m) = N*base_l + (n*(2l+1)+m)*W_l + u'
 * (W_l = mul_l, or 2 mul_l for the U|V pair buffer).  Each block is a plain row-major
 * [N(2l+1), W_l] matrix, so o3.Linear (nn/xpainn.py:186-187, 211-212) is three ordinary GEMMs. */

/* nn.LayerNorm(s) (nn/xpainn.py:123,130) + EquivariantLayerNorm(x) (nn/o3layer.py:145-171) in one
 * pass; shat has row stride ld_s, xhat is written in BT layout, stats[N,4] = (mean, rstd, mean0, r).
 * do_norm = 0: identity norms (layer_norm=False), still re-laying x out. */
int xeq_norm_fwd(int dtype, const void* s, const void* x, const void* ln_w, const void* ln_b, const void* eq_w,
                 const void* eq_b, int64_t n, int node_dim, const int32_t mul[3], int do_norm, void* shat, int64_t ld_s,
                 void* xhat_bt, void* stats, void* stream);
/* g_s = res_s + LN^T g_shat ; g_x = res_x + EqLN^T g_xhat_bt  (res_* may be NULL; g_x in e3nn layout). */
int xeq_norm_bwd(int dtype, const void* s, const void* x, const void* ln_w, const void* eq_w, const void* stats,
                 int64_t n, int node_dim, const int32_t mul[3], int do_norm, const void* g_shat, int64_t ld_gs,
                 const void* g_xhat_bt, const void* res_s, const void* res_x, void* g_s, void* g_x, void* stream);
/* Invariant(V) and EquivariantDot(U,V) (nn/xpainn.py:214,222; nn/o3layer.py:39-44,104-109) from the U|V
 * pair buffer: cat[n, node_dim + u] = sqrt(sum_m V^2 + eps^2) - eps, p[n,u] = sum_m U V; and the reverse. */
int xeq_uv_reduce_fwd(int dtype, const void* uv_bt, int64_t n, const int32_t mul[3], double eps, void* cat,
                      int64_t ld_cat, int node_dim, void* p, void* stream);
/* Reverse: g_U = dL/dU of the output stage + g_p V, g_V = g_p U + g_v V / (v + eps).  The output stage's part is formed
 * here as g_x_out[n,u,m] * a_vv[n,u] when g_x_out / a are given (then xeq_update_out_bwd is called with g_uv_bt = NULL);
 * with both NULL it is read from the U columns of g_uv_bt, where xeq_update_out_bwd left it. */
int xeq_uv_reduce_bwd(int dtype, const void* uv_bt, const void* g_p, const void* g_cat, int64_t ld_cat, int node_dim,
                      int64_t n, const int32_t mul[3], double eps, const void* g_x_out, const void* a, void* g_uv_bt,
                      void* stream);
/* Charge / spin embeddings of XPaiNN (nn/electronic.py:13-90 with the bias-free ResidualLayer of nn/basic.py:11-31; inserted between
 * the embedding and the first message block by nn/model.py:85-96), f32, csrc/xeq_electronic.hip.  kind 0: ChargeEmbedding, a_g =
 * relu([t_g, -t_g]); kind 1: SpinEmbedding, a_g = [t_g]; total[G] (f32) holds t_g per graph.  With key_in = a_g / max(a_g, 1):
 *   attn_n = softplus(<W_q s_n + b_q, W_k key_in(g(n))> / sqrt(F)),  c_n = attn_n (W_v a_g(n)) / sum_{m in g(n)} attn_m,
 *   out_n = s_n + (c_n + SiLU(W_2 SiLU(W_1 c_n))) / sqrt(2).
 * Two launches (xeq_electronic_attn, xeq_electronic_mix).  s [n, lds] (lds % 4 == 0), ptr [G + 1] (int64, graph g = atoms ptr[g] ..
 * ptr[g + 1] - 1), wq_packed = xeq_mlp_pack(W_q, b_q, F, F, 0), w_k / w_v the nn.Linear weights [F, 2] (charge) or [F, 1] (spin),
 * w1_packed / w2_packed = xeq_mlp_pack(residual.mlp.{0,2}.weight, NULL, F, F, 0); attn [n] is workspace; out [n, F] must not overlap s.
 * The graph sums run in an order fixed by the graph's own atoms, without atomics: a molecule gets the same bits alone, in a batch or
 * in a shard.  xeq_electronic_supported: f32, node_dim a multiple of 32, <= 256 (1 / 0, not a status). */
int xeq_electronic_supported(int dtype, int node_dim);
int xeq_electronic_fwd(int kind, const void* s, int64_t lds, int64_t n, int node_dim, const int64_t* ptr, int64_t n_graphs, const void* total,
                       const void* wq_packed, const void* w_k, const void* w_v, const void* w1_packed, const void* w2_packed, void* attn,
                       void* out, void* stream);

/* Output stage of XPainnUpdate (nn/xpainn.py:218-229) with a = [a_vv C | a_sv F | a_ss F], ip = dot_lin(p):
 * s_out = s + a_sv*ip + a_ss, x_out = x + U (x) a_vv (x, x_out in e3nn layout; x_out may be NULL: not computed); and the reverse
 * (g_uv_bt may be NULL: dL/dU = g_x_out a_vv is then left to xeq_uv_reduce_bwd; g_x_out may be NULL: zero). */
int xeq_update_out_fwd(int dtype, const void* s, const void* x, const void* uv_bt, const void* a, const void* ip,
                       int64_t n, int node_dim, const int32_t mul[3], void* s_out, void* x_out, void* stream);
int xeq_update_out_bwd(int dtype, const void* g_s_out, const void* g_x_out, const void* uv_bt, const void* a,
                       const void* ip, int64_t n, int node_dim, const int32_t mul[3], void* g_a, void* g_ip,
                       void* g_uv_bt, void* stream);

/* ---- two-layer scalar MLPs on the matrix cores (f32; hidden width 128: xeq_mlp2_*, 32 .. 256: xeq_mlp2h_*) ----
 * Replace nn.Sequential(Linear, SiLU, Linear) of XPainnMessage.scalar_mlp (nn/xpainn.py:103-107) and
 * XPainnUpdate.update_mlp (nn/xpainn.py:177-181) and their input gradients: one launch each, the hidden
 * activations stay on chip.  Weights are read from a packed copy in matrix-core fragment order with the bias as one
 * more k-group (xeq_mlp_pack; xeq_mlp_packed_floats(n_out, k_in) floats):
 *   packed W1  = pack(lin1.weight [128, k1], lin1.bias, transposed = 0)     forward stage 1
 *   packed W2  = pack(lin2.weight [n2, 128], lin2.bias, transposed = 0)     forward stage 2
 *   packed W2t = pack(lin2.weight viewed as [k_in = n2][n_out = 128], NULL, transposed = 1)   reverse stage 1
 *   packed W1t = pack(lin1.weight viewed as [k_in = 128][n_out = k1], NULL, transposed = 1)   reverse stage 2
 * xeq_mlp2_supported: 1 when the kernels take (dtype, k1, hidden, n2): f32, hidden 128, k1 % 32 == 0 (it is the
 * reverse pass's output width), n2 % 32 == 0. */
int xeq_mlp2_supported(int dtype, int k1, int hidden, int n2);
/* Work split of the node kernels (host logic): out = {tiles with one workgroup each, workgroups per remaining tile, grid size}
 * for `tiles` 32-node tiles whose second phase can be cut in at most `max_split` pieces. */
int xeq_node_tile_split(int64_t tiles, int max_split, int64_t out[3]);
int64_t xeq_mlp_packed_floats(int n_out, int k_in);
int xeq_mlp_pack(const float* w, const float* bias, int n_out, int k_in, int transposed, float* packed, void* stream);
/* y[n, n2] (row stride ldy, % 4 == 0) = silu(x[n, k1] (row stride ldx, % 4 == 0) W1^T + b1) W2^T + b2;
 * pre[n, 128] = the pre-activation, kept for the reverse pass. */
int xeq_mlp2_fwd(const float* x, int64_t ldx, int64_t n, int k1, const float* w1_packed, const float* w2_packed, int n2,
                 float* pre, float* y, int64_t ldy, void* stream);
/* gx[n, n2] = ((g[n, k1] W2) * silu'(pre)) W1 with k1 = the forward's n2 and n2 = the forward's k1. */
int xeq_mlp2_bwd(const float* g, int64_t ldg, int64_t n, int k1, const float* w2t_packed, const float* pre,
                 const float* w1t_packed, int n2, float* gx, int64_t ldgx, void* stream);
/* The same two products with the hidden width given at the call: `hidden` = 32, 64, ..., 256 (the node_dim the message, PaiNN,
 * electronic and head kernels take), k1 % 32 == 0, n2 % 32 == 0, f32 (`dtype` is checked, not dispatched on), row strides % 4 == 0.
 * xeq_mlp2h_supported answers 1 exactly there; outside it _fwd / _bwd return XEQ_ERR_INVALID_ARGUMENT with a message and launch
 * nothing.  The packed copies are those above with 128 replaced by `hidden`; pre is [n, hidden].  hidden == 128 IS xeq_mlp2_fwd /
 * _bwd (same kernels, launch name and bits).  The other widths run one 32-row kernel at every row count (few rows are shared among
 * workgroups by output tile), recorded as xeq_mlp2h_fwd / xeq_mlp2h_bwd: a row's bits depend on neither the row count nor the
 * workgroup that computed it, and per element the sums are taken in the order of the 128-wide kernels. */
int xeq_mlp2h_supported(int dtype, int k1, int hidden, int n2);
int xeq_mlp2h_fwd(int dtype, const float* x, int64_t ldx, int64_t n, int k1, int hidden, const float* w1_packed, const float* w2_packed, int n2,
                  float* pre, float* y, int64_t ldy, void* stream);
int xeq_mlp2h_bwd(int dtype, const float* g, int64_t ldg, int64_t n, int k1, int hidden, const float* w2t_packed, const float* pre,
                  const float* w1t_packed, int n2, float* gx, int64_t ldgx, void* stream);
/* XPainnUpdate's two independent products side by side (reference nn/xpainn.py:219-223: a = update_mlp([shat | v]) and dot_lin(<U, V>);
 * reverse = 1: their input gradients): xeq_mlp2_fwd (reverse: xeq_mlp2_bwd with stage1_packed = w2t_packed, stage2_packed = w1t_packed)
 * and xeq_linear_fwd without bias / activation / row gather on the same n rows.  One launch when n takes the few-row forms
 * (XEQ_SMALL_ROWS, csrc/xeq_common.h), else the two launches in this order.  The same bits as the separate entry points.  Hidden width 128 only: at the other
 * widths the callers issue xeq_mlp2h_fwd / _bwd and xeq_linear_fwd themselves. */
int xeq_mlp2_and_linear(int reverse, const float* x, int64_t ldx, int64_t n, int k1, const float* stage1_packed, const float* stage2_packed,
                        int n2, float* pre, float* y, int64_t ldy, const float* lin_x, int64_t lin_ldx, int lin_k,
                        const float* lin_w_packed, int lin_n_out, float* lin_y, int64_t lin_ldy, void* stream);

/* ---- first half of XPainnUpdate.forward in one launch (f32; mul_l in {0, 32, 64, 128}, node_dim % 4 == 0, <= 128, D <= 480) ---
 * nn.LayerNorm(s) and EquivariantLayerNorm(x) (nn/xpainn.py:208-209), U = update_U(xhat), V = update_V(xhat) (o3.Linear,
 * nn/xpainn.py:211-212), v = Invariant(V), p = EquivariantDot(U, V) (nn/xpainn.py:214, :222).  Replaces xeq_norm_fwd + the
 * three GEMMs + xeq_uv_reduce_fwd; outputs as theirs: cat[n, :node_dim] = shat, cat[n, node_dim:node_dim + C] = v (row stride
 * ld_cat), p[n, C], the U|V pair buffer uv_bt (BT layout), stats[n, 4].  w_packed_l = xeq_mlp_pack([W_U | W_V] / sqrt(mul_l)
 * viewed [k_in = mul_l][n_out = 2 mul_l], bias = [b_U | b_V] for l = 0 (has_bias) else NULL, transposed = 1); NULL for an
 * absent block.  xeq_update_uv_supported: 1 when the kernel takes the layout. */
int xeq_update_uv_supported(int dtype, int node_dim, const int32_t mul[3]);
int xeq_update_uv_fwd(const float* s, const float* x, const float* ln_w, const float* ln_b, const float* eq_w, const float* eq_b,
                      int64_t n, int node_dim, const int32_t mul[3], int do_norm, const float* w_packed0, const float* w_packed1,
                      const float* w_packed2, int has_bias, double eps, float* cat, int64_t ld_cat, float* p, float* uv_bt,
                      float* stats, void* stream);
/* Reverse of the above in one launch (replaces xeq_uv_reduce_bwd + three GEMMs + xeq_norm_bwd):
 *   g_U = g_x_out a_vv + g_p V,  g_V = g_p U + g_v V / sqrt(sum_m V^2 + eps^2)   (g_v = g_cat[:, node_dim:], a_vv = a[:, :C])
 *   g_xhat = g_U W_U^T + g_V W_V^T;  g_s = g_s_out + LN^T(g_cat[:, :node_dim]),  g_x = g_x_out + EqLN^T(g_xhat).
 * wt_packed_l = xeq_mlp_pack([W_U | W_V] / sqrt(mul_l) as [n_out = mul_l][k_in = 2 mul_l], NULL, transposed = 0).
 * g_x_out may be NULL (the block's equivariant output has no consumer: the last block of a force evaluation): zero.
 * Split form (g_xhat_bt != NULL): stops after the contraction and writes dL/dxhat in BT layout for xeq_norm_bwd (g_s_out, s,
 * x, stats, ln_w, eq_w, g_s, g_x unused; the workgroup then needs 50 KB of LDS instead of 113 KB). */
int xeq_update_uv_bwd(const float* uv_bt, const float* g_p, const float* g_cat, int64_t ld_cat, const float* g_x_out,
                      const float* g_s_out, const float* a, int64_t ld_a, const float* s, const float* x, const float* stats,
                      const float* ln_w, const float* eq_w, int64_t n, int node_dim, const int32_t mul[3], int do_norm,
                      const float* wt_packed0, const float* wt_packed1, const float* wt_packed2, double eps, float* g_s, float* g_x,
                      float* g_xhat_bt, void* stream);

/* Epoch of the packed weight copies: every pack cache (nn/fused.py, nn/nodeblock.py, csrc/xeq_torch.cpp) keys on it next to the version
 * counters of the tensors it packed; what changes parameters without bumping those counters (a replayed captured optimizer step,
 * train.GraphedTrainStep) calls xeq_pack_epoch_bump and the next evaluation repacks.  Host only. */
long long xeq_pack_epoch(void);
void xeq_pack_epoch_bump(void);
/* Capacity form of the open-boundary list: count[0] = raw[n_nodes] (the true edge count); rowptr = raw when the list fits `capacity`,
 * all zeros (an EMPTY list) when it does not -- a cut list would not be symmetric and the symmetric shortcuts downstream index by the
 * reverse edge (replaces the unguarded row pointer of round 3: a list that outgrew its arrays now leads no kernel past a buffer). */
int xeq_rowptr_guard(const int32_t* raw, int64_t n_nodes, int64_t capacity, int32_t* rowptr, int32_t* count, void* stream);
/* Degrees -> guarded row pointer in ONE launch (round 5): rowptr[0 .. n] = exclusive prefix sums of deg[0 .. n) with
 * xeq_rowptr_guard's rule (a list beyond `capacity` becomes EMPTY; capacity < 0: no guard), count[0] (optional) = the true total,
 * running_total[0] (optional, int64) += the true total: a device-side counter of the edges a replayed step has processed.
 * One workgroup; n_nodes <= xeq_rowptr_from_degrees_max() (XEQ_ERR_UNSUPPORTED above: xeq_exclusive_scan_i32_ws + xeq_rowptr_guard). */
int xeq_rowptr_from_degrees(const int32_t* deg, int64_t n_nodes, int64_t capacity, int32_t* rowptr, int32_t* count, int64_t* running_total,
                            void* stream);
int64_t xeq_rowptr_from_degrees_max(void);   /* a size, not a status */

/* ---- the per-node chain between two message aggregations as ONE launch per direction (round 4; csrc/xeq_nodeblock.hip) -------------
 * f32, the default layout (node_dim 128, 128x0e + 64x1o + 32x2e: xeq_node_block_supported).  A wave owns 16 nodes and keeps their
 * activations in the matrix cores' accumulator layout; every contraction runs on bf16 MFMAs (16x16x32) over three-way split operands
 * (six products per k-step, f32 accumulation); the weights stream through LDS from a copy packed in consumption order.
 *
 * xeq_node_block_fwd = XPainnUpdate.forward (nn/xpainn.py:206-231: both norms, o3.Linear U / V, Invariant, EquivariantDot, update_mlp,
 * dot_lin, residual update) and, when h_next != NULL, the front half of the NEXT XPainnMessage.forward (nn/xpainn.py:128-139: both
 * norms of (s_out, x_out) and scalar_mlp).  It replaces xeq_update_uv_fwd + xeq_mlp2_fwd + xeq_linear_fwd + xeq_update_out_fwd
 * (+ xeq_norm_fwd + xeq_mlp2_fwd of the next block).  What other kernels read keeps their layouts: s_out [n, F], x_out [n, D] (NULL: no
 * consumer), stats [n, 4], and for the next block stats_next [n, 4], xhat_next (BT), h_next [n, F + 2 C].  What only the reverse launch
 * reads is INTERNAL: uv (U|V), pre (update_mlp hidden pre-activation), a (update_mlp output), ip (dot_lin output), pre_next and the
 * scratch p -- xeq_node_block_rows(n) rows each (whole workgroups of 64 nodes) in the wave-native layout [block of 16 nodes][tile of
 * 32 channels][register quad g][lane = 16 q + node][4 floats] (channel 16 g + 4 q + e of the tile), in which every wave access is 1 KB of consecutive bytes (tile numbering:
 * csrc/xeq_nodeblock.hip, uv_tile / x_tile; nn/nodeblock.py::native_to_rows turns one into rows).
 * packed: xeq_node_block_pack_fwd(update_mlp[0].weight [F, F + C], [W_U | W_V] / sqrt(mul_l) as [mul_l, 2 mul_l] for l = 0, 1, 2,
 * dot_lin.weight [F, C], update_mlp[2].weight [C + 2 F, F], next scalar_mlp[0].weight [F, F] and [2].weight [F + 2 C, F] (both
 * NULL: without the next block), out, stream); out holds xeq_node_block_fwd_tiles(with_tail) * 3072 bytes.
 * b_uv = [update_U.bias | update_V.bias] ([2 F]) or NULL; p_scratch: [n, C] floats (EquivariantDot(U, V), read back by dot_lin). */
int xeq_node_block_supported(int dtype, int node_dim, const int32_t mul[3]);
/* launch policy (host only): 1 when an evaluation of n nodes should take the fused launches (n >= XEQ_NODE_BLOCK_MIN_NODES, default
 * 6 144; XEQ_NODE_BLOCK=0: never).  Below that the chain of small kernels is faster (a fused launch is one serial chain per wave). */
int xeq_node_block_auto(int64_t n);
/* launch policy (host only): the row count up to which xeq_linear_fwd, xeq_mlp2_fwd / _bwd, xeq_mlp2_and_linear and xeq_update_uv_fwd /
 * _bwd (split form) take their few-row forms -- 16 x 16 exact-f32 tiles whose results equal the 32-row kernels' bit for bit (MD-sized
 * systems: a quarter of the k-chain per wave, four times the waves).  3 584; XEQ_SMALL_ROWS overrides (0: never), read per call. */
int64_t xeq_small_rows_limit(void);
/* waves per workgroup of the node-block launches that follow (host only, process-wide): 0 = by node count (one workgroup per CU of 5 .. 8
 * waves between 4 097 and 8 192 wave-blocks of 16 nodes, four otherwise: a lone launch ends with its slowest CU), 4 .. 8 = fixed.  Results
 * do not depend on it.  -> the former setting; -1: out of range, nothing changed. */
int xeq_node_block_set_waves(int waves);
int64_t xeq_node_block_rows(int64_t n);
int64_t xeq_node_block_fwd_tiles(int with_tail);
int xeq_node_block_pack_fwd(const float* w3, const float* uv0, const float* uv1, const float* uv2, const float* dot, const float* w4,
                            const float* w1_next, const float* w2_next, void* out, void* stream);
int xeq_node_block_fwd(int64_t n, const float* s, const float* x, const float* ln_w, const float* ln_b, const float* eq_w, const float* eq_b,
                       const float* b_uv, const float* b3, const float* b4, double eps, const void* packed, float* p_scratch, float* uv_bt, float* stats,
                       float* pre, float* a, float* ip, float* s_out, float* x_out, const float* ln_w_next, const float* ln_b_next,
                       const float* eq_w_next, const float* eq_b_next, const float* b1_next, const float* b2_next, float* stats_next,
                       float* xhat_next, float* pre_next, float* h_next, void* stream);
/* Reverse of xeq_node_block_fwd for a force evaluation (input gradients only, nn/basic.py:143-159): replaces xeq_mlp2_bwd + xeq_norm_bwd
 * of the next message block and xeq_update_out_bwd + xeq_linear_fwd (dot_lin^T) + xeq_mlp2_bwd + xeq_update_uv_bwd + xeq_norm_bwd of the
 * update block.  With the next block's front half (g_h != NULL): g_h [n, F + 2 C] and g_xhat_next (BT) are the gradients of h_next /
 * xhat_next, g_s_in / g_x_in the gradients that reach s_out / x_out directly (the message kernel's residual path), and s_out, x_out,
 * stats_next, pre_next what the forward launch wrote.  Without it: g_s_in = dL/ds_out, g_x_in = dL/dx_out or NULL (zero: the last
 * block of a force evaluation; packed with with_gx = 0).  Scratch (caller-owned, xeq_node_block_rows(n) rows each, internal layout):
 * gxo [., D] (whenever dL/dx_out is not zero), gp [., C], gv [., C], gw [., D].  Output: g_s [n, F], g_x [n, D].  packed: xeq_node_block_pack_bwd of the same weight tensors as the forward pack. */
int64_t xeq_node_block_bwd_tiles(int with_tail, int with_gx);
int xeq_node_block_pack_bwd(const float* w3, const float* uv0, const float* uv1, const float* uv2, const float* dot, const float* w4,
                            const float* w1_next, const float* w2_next, int with_gx, void* out, void* stream);
int xeq_node_block_bwd(int64_t n, const float* g_h, const float* g_xhat_next, const float* g_s_in, const float* g_x_in, const float* s_out,
                       const float* x_out, const float* stats_next, const float* pre_next, const float* ln_w_next, const float* eq_w_next,
                       const float* uv_bt, const float* a, const float* ip, const float* pre, const float* s, const float* x,
                       const float* stats, const float* ln_w, const float* eq_w, double eps, const void* packed, float* gxo, float* gp,
                       float* gv, float* gw, float* g_s, float* g_x, void* stream);
/* test entry: y [n, 32 n_ot] = x [n, 128] W^T (W [32 n_ot, 128]) through the kernel's primitives; form 0 (n_ot = 4): chunk
 * accumulation, form 1: one output tile at a time; packed_scratch: 8 n_ot * 3072 bytes */
int xeq_node_block_linear_test(const float* x, int64_t n, const float* w, int n_ot, int form, void* packed_scratch, float* y, void* stream);

/* ---- PaiNN (nn/painn.py of the reference; csrc/xeq_painn.hip) -----------------------------------------------------------------------
 * f32; node_dim F a multiple of 32 up to 256, num_basis <= 31.  Node scalars s [n, F], node vectors x [n, 3, F] Cartesian (x, y, z).
 * Every product is the exact-f32 matrix instruction: a row's bits do not depend on the batch around it.
 * xeq_painn_supported -> 1 / 0.  xeq_painn_few_rows_limit: node count up to which the update products launch one wave per workgroup
 * (one workgroup per 16 nodes x 16 output columns; same bits as the four-wave form). */
int xeq_painn_supported(int dtype, int node_dim, int num_basis);
int64_t xeq_painn_few_rows_limit(void);
/* packed copies (caller-owned): the filter rbf_lin (weight [3 F, B], bias [3 F]) as [32, 3 F] with the bias in row B; update_U / update_V
 * (weights [F, F], no bias) as four matrices in operand order (forward pair, reverse pair). */
int64_t xeq_painn_filter_packed_floats(int node_dim);
int64_t xeq_painn_uv_packed_floats(int node_dim);
int xeq_painn_pack_filter(const float* w, const float* b, int node_dim, int num_basis, float* out, void* stream);
int xeq_painn_pack_uv(const float* wu, const float* wv, int node_dim, float* out, void* stream);
/* Message block, nn/painn.py:100-117 (h [n, 3 F] = scalar_mlp(s) of :99 comes from xeq_mlp2_fwd): one wave per center walks
 * rowptr / perm (center-sorted CSR of edge_index [2, E], perm NULL: already sorted) in chunks of 16 edges; radial basis (p0, p1 as
 * xeq_message_fwd), envelope and unit vectors are formed per chunk on chip from vec [E, 3]; s_out = s + sum m_s,
 * x_out[c] = x[c] + sum (x[nbr, c] gate_state + u_c gate_edge): one store per node, no atomics. */
int xeq_painn_message_fwd(int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* perm, const int64_t* edge_index, const float* vec,
                          const float* h, const float* s, const float* x, const float* w_packed, const float* p0, const float* p1, int rbf_kind,
                          int cutoff_kind, int num_basis, double cutoff, int node_dim, float* s_out, float* x_out, void* stream);
/* Reverse of nn/painn.py:100-117: one wave per NEIGHBOUR walks n_rowptr / n_perm (the reverse-edge map of a symmetric list, or the
 * neighbour-sorted view).  g_s [n, F], g_x [n, 3, F] or NULL (zero) are dL/ds_out, dL/dx_out.  Outputs: g_h [n, 3 F]; g_x_in [n, 3, F]
 * (residual included) or NULL (not wanted); g_vec [E, 3] = dL/dvec through basis, envelope and u = r / d (zero subgradient at r = 0),
 * written (accumulate_vec = 0) or added to (1: the blocks of one evaluation share the buffer that feeds xeq_edge_vectors_bwd).
 * dL/ds is g_s + the reverse of the scalar MLP on g_h (xeq_mlp2_bwd, xeq_painn_add). */
int xeq_painn_message_bwd(int64_t n_nodes, int64_t n_edges, const int32_t* n_rowptr, const int32_t* n_perm, const int64_t* edge_index, const float* vec,
                          const float* h, const float* x, const float* w_packed, const float* p0, const float* p1, int rbf_kind, int cutoff_kind,
                          int num_basis, double cutoff, int node_dim, const float* g_s, const float* g_x, float* g_h, float* g_x_in, float* g_vec,
                          int accumulate_vec, void* stream);
/* Update block, nn/painn.py:146-164.  uv_fwd (:149-153): U, V [n, 3, F] = x W^T, ip [n, F] = <U, V>, cat [n, 2 F] = [s | |V|] (plain
 * Euclidean norm), the input of update_mlp (xeq_mlp2_fwd -> a [n, 3 F] = a_ss | a_vv | a_sv).  out_fwd (:156-164): s_out = s + a_sv ip
 * + a_ss, x_out = x + a_vv U (x_out NULL: not formed).  out_bwd: g_a [n, 3 F] from g_s, g_x (NULL: zero).  uv_bwd: g_cat [n, 2 F] is
 * xeq_mlp2_bwd of g_a; g_s_in = g_s + g_cat[:, :F]; g_x_in = g_x + dL/dU W_U + dL/dV W_V, the norm's gradient exactly 0 where |V| = 0. */
int xeq_painn_update_uv_fwd(int64_t n, int node_dim, const float* s, const float* x, const float* uv_packed, float* U, float* V, float* ip, float* cat,
                            void* stream);
int xeq_painn_update_out_fwd(int64_t n, int node_dim, const float* s, const float* x, const float* a, const float* U, const float* ip, float* s_out,
                             float* x_out, void* stream);
int xeq_painn_update_out_bwd(int64_t n, int node_dim, const float* g_s, const float* g_x, const float* U, const float* ip, float* g_a, void* stream);
int xeq_painn_update_uv_bwd(int64_t n, int node_dim, const float* g_s, const float* g_x, const float* a, const float* U, const float* V, const float* cat,
                            const float* g_cat, const float* uv_packed, float* g_s_in, float* g_x_in, void* stream);
/* out = a + b (n floats): the two paths of dL/ds behind a message block */
int xeq_painn_add(const float* a, const float* b, int64_t n, float* out, void* stream);

/* Property heads of XPaiNN (nn/output.py:28-76 ScalarOut, :131-179 AtomicChargesOut, :245-326 PolarOut), f32 inference,
 * csrc/xeq_heads.hip.  The scalar and charge MLPs run on the energy head's kernels (xeq_head_fwd / xeq_linear_fwd + xeq_head_dot).
 * xeq_head_polar_nodes: PolarOut per node in one launch over tiles of 32 nodes,
 *   t[n] = (a0 t0, a2 t2[0..5), 0, 0),  (a0, a2) = scalar_out_mlp(s_n),  (t0, t2) = equi_out_mlp(x_n) (o3.Linear - Gate - o3.Linear;
 *   the gate is sigmoid(sqrt(sum_m h^2 + eps^2) - eps) per channel; the 1o block of x is not read).
 * s [n, lds], x [n, ldx] with the 0e block at column 0 and the 2e block at column off2 (strides and off2 multiples of 4, buffers
 * 16-byte aligned); rows past n are neither read nor written.  The three hidden products are exact-f32 matrix-core tiles:
 * ws1_packed = xeq_mlp_pack(scalar_out_mlp.0.weight, bias) with hidden_dim rounded up to a multiple of 32 by zero rows,
 * w0_packed / w2_packed the same for the 0e / 2e blocks of equi_out_mlp.0.weight, transposed to [mul_out, mul_in] and scaled by
 * 1 / sqrt(mul_in) (the 0e copy carries the o3 bias, the 2e copy none).  ws2 [2, hidden_dim], bs2 [2], wb [hid0 + hid2] (flat
 * equi_out_mlp.2.weight), bb [1].  t [n, 8]: six values and two zeros.
 * xeq_head_polar_supported (1 / 0, not a status): f32 (SiLU is the only activation); node_dim, mul0 multiples of 32, <= 256; mul2 a
 * multiple of 8, <= 64; hidden_dim, hid0 multiples of 4, <= 128; hid2 a multiple of 4, <= 32; the tile's LDS within 160 KB.
 * xeq_head_graph_reduce: per graph g the sum of `width` (<= 8) columns of src rows ptr[g] .. ptr[g + 1] - 1, one wave per graph, lane
 * l adding rows ptr[g] + l, + 64, ... and a fixed butterfly -- no atomics, the order depends on the atom's index in its graph alone,
 * so a graph's result is bit-identical alone, in a batch and in a shard.  mode 0: out [G, width] = sum; 1: mean; 2 (width 6): out
 * [G, 9] = z I + A of nn/output.py:301-320 and iso [G] = tr / 3 when iso is given; 3 (width 1): src[i] += (total[g] - sum) / n_g
 * over the graph's rows (total NULL: zero).  An empty graph gives zeros and divides nothing.  Neither entry has a reverse pass. */
int xeq_head_polar_supported(int dtype, int node_dim, int mul0, int mul2, int hidden_dim, int hid0, int hid2);
int xeq_head_polar_nodes(const void* s, int64_t lds, const void* x, int64_t ldx, int64_t n, int node_dim, int mul0, int mul2, int off2,
                         int hidden_dim, int hid0, int hid2, const void* ws1_packed, const void* w0_packed, const void* w2_packed,
                         const void* ws2, const void* bs2, const void* wb, const void* bb, double eps, void* t, void* stream);
int xeq_head_graph_reduce(int mode, void* src, int64_t ld, int width, const int64_t* ptr, int64_t n_graphs, const void* total, void* out,
                          void* iso, void* stream);

/* Ewald message passing (nn/ewald.py:141-212 EwaldBlock behind the geometry of :60-138), f32 inference with an explicit reverse pass,
 * csrc/xeq_ewald.hip.  Atom n of graph g (ptr [G + 1], ptr[0] = 0, ptr[G] = n) at pos [n, 3]; kvec [G, K, 3] with kvec_gstride floats
 * between two graphs' tables (0: one [K, 3] table for every graph); theta_nk = <kvec[g, k], pos_n>, computed in the kernels in f32 with
 * the accurate sincosf; damp [n] the per-atom damping d_n (NULL: 1).  Every contraction runs on the exact-f32 matrix instruction.  No
 * float atomics: a graph is cut into chunks of xeq_ewald_chunk() atoms counted from its first atom and the chunk partials are added in
 * chunk order, so a graph's results are bit-identical alone, inside any batch, in a shard and on repeat.  K is padded to the tile
 * inside the kernels; empty graphs give zeros.
 * xeq_ewald_supported (1 / 0, not a status): f32; node_dim a multiple of 32, <= 256; 1 <= n_k <= 192.
 * xeq_ewald_structure_factor: s_r[g, k, f] = sum_{n in g} d_n cos(theta_nk) x[n, f], s_i with sin ([G, K, node_dim], every entry
 *   written).  x [n, ldx] (ldx a multiple of 4, 16-byte aligned); parts: workspace of xeq_ewald_parts_floats(n, G, n_k, node_dim) floats
 *   (0 when no graph can exceed one chunk: parts may be NULL).
 * xeq_ewald_apply: out[n, f] = d_n sum_k kf[k, f] (cos(theta_nk) s_r[g, k, f] + sin(theta_nk) s_i[g, k, f]); kf [n_k, node_dim], out
 *   [n, ldo].  The operator x -> out of the two entries in sequence is symmetric: applied to dL/dout it gives dL/dx.
 * xeq_ewald_phase_grad: with (s_r, s_i) the structure factors of h and (p_r, p_i) those of gm = dL/dout,
 *   T1[n, k] = sum_f kf[k, f] (gm[n, f] s_r[g, k, f] + h[n, f] p_r[g, k, f]), T2 with the imaginary parts,
 *   g_theta[n, k] = d_n (-sin T1 + cos T2) ([n, n_k], optional), g_damp[n] = sum_k (cos T1 + sin T2) (optional),
 *   g_pos[n, :] = sum_k g_theta[n, k] kvec[g, k, :] + g_damp[n] ddamp[n, :] (ddamp [n, 3] = dd_n / dpos_n, NULL: no such term).
 *   dL/dkf and dL/dkvec are not formed (inference).
 * Row kernels of the block's glue: xeq_ewald_damping: damp[n] = prod_i sinc(scale pos[n, i] + eps) (torch.sinc) and ddamp [n, 3]
 * (optional); xeq_ewald_layernorm_fwd / _bwd: LayerNorm over node_dim (<= 256) on contiguous rows, stats [n, 2] = (mean, rstd);
 * xeq_ewald_combine: out = (sa a + sb b) [* silu'(pre)] over `count` floats (b, pre optional). */
int xeq_ewald_supported(int dtype, int node_dim, int n_k);
int64_t xeq_ewald_chunk(void);
int64_t xeq_ewald_parts_floats(int64_t n, int64_t n_graphs, int n_k, int node_dim);
int xeq_ewald_structure_factor(const void* x, int64_t ldx, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride, int n_k,
                               const void* damp, const int64_t* ptr, int64_t n_graphs, void* parts, void* s_r, void* s_i, void* stream);
int xeq_ewald_apply(const void* s_r, const void* s_i, const void* kf, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride,
                    int n_k, const void* damp, const int64_t* ptr, int64_t n_graphs, void* out, int64_t ldo, void* stream);
int xeq_ewald_phase_grad(const void* gm, int64_t ldg, const void* h, int64_t ldh, const void* s_r, const void* s_i, const void* p_r, const void* p_i,
                         const void* kf, int64_t n, int node_dim, const void* pos, const void* kvec, int64_t kvec_gstride, int n_k, const void* damp,
                         const void* ddamp, const int64_t* ptr, int64_t n_graphs, void* g_theta, void* g_damp, void* g_pos, void* stream);
int xeq_ewald_damping(const void* pos, int64_t n, double scale, double eps, void* damp, void* ddamp, void* stream);
int xeq_ewald_layernorm_fwd(const void* x, int64_t n, int node_dim, const void* weight, const void* bias, double eps, void* y, void* stats, void* stream);
int xeq_ewald_layernorm_bwd(const void* g, const void* x, const void* stats, const void* weight, int64_t n, int node_dim, void* g_x, void* stream);
int xeq_ewald_combine(const void* a, double sa, const void* b, double sb, const void* pre, int64_t count, void* out, void* stream);

/* Device-resident drivers around a whole-step graph (xequinet_amd/resident.py, csrc/xeq_md.hip): molecular dynamics (md.py, DESIGN.md
 * sections 12, 15 and 17) and batched FIRE and L-BFGS geometry optimisation (optimize.py, sections 13 and 16), f32 / f64.  One step is a FRONT entry, the step's
 * graph on the step object's static buffers, a BACK entry; nothing reaches the host between them.
 *
 * The entries take their arguments as RECORDS, by pointer: what every driver has (the system, the step graph's outputs, the chunk
 * tables, the recorder) and one record of parameters per driver.  Every member is 8 bytes wide -- a pointer, int64_t, uint64_t or double
 * -- so a record's layout is its field order, without padding, on any ABI; xeq_record_bytes(which) gives the library's sizeof for a
 * binding to compare with its own (-1: no such record).  A record is read during the call and not retained.  Pointers are device
 * pointers unless marked HOST; `dtype` below: a buffer of the system record's floating type. */
enum { XEQ_REC_SYSTEM = 0, XEQ_REC_STEP = 1, XEQ_REC_CHUNKS = 2, XEQ_REC_RECORDER = 3, XEQ_REC_MD = 4, XEQ_REC_NPT = 5, XEQ_REC_FIRE = 6,
       XEQ_REC_NEIGHBORS = 7 /* xeq_neighbor_search, with the neighbour search above */, XEQ_REC_LBFGS = 8 };
int64_t xeq_record_bytes(int which);

typedef struct xeq_res_system {
  int64_t dtype;        /* XEQ_F32 / XEQ_F64 */
  int64_t n;            /* atoms */
  int64_t n_graphs;     /* graphs (the barostat's entries serve ONE box and do not read it) */
  int64_t n_chunks;     /* entries of the chunk tables (xeq_res_chunks) */
  void* pos;            /* [n, 3] `dtype`: the step object's static positions; a front updates pos, vel and image in place */
  void* vel;            /* [n, 3] `dtype` */
  void* frc;            /* [n, 3] `dtype`: the driver's forces, written by a back from frc_step */
  int32_t* image;       /* [n, 3]: the periodic images an atom has crossed, kept by the wrap; needed with a cell and a periodic axis */
  const int64_t* batch; /* [n]: the atom's graph */
  int64_t* book;        /* int64 [4] = {steps done (FIRE: evaluations done), largest n_edges seen, non-finite flag, xeq_npt_back's image flag
                           (FIRE: graphs not converged)}, maintained by the back entries with plain stores of one lane; the host resets
                           entries 1 and 2 when it has read them */
  const double* cell;   /* HOST: 9 doubles, rows = lattice vectors; NULL for open boundaries (the barostat's box is on the device:
                           xeq_npt_params.box, and its entries read neither this nor pbc) */
  const int32_t* pbc;   /* HOST: 3 int32; NULL for open boundaries */
} xeq_res_system;

/* The step graph's outputs and what it was captured with: the part that changes on a re-capture. */
typedef struct xeq_res_step {
  const void* frc_step;        /* [n, 3] `dtype` */
  const void* energy_step;     /* [n_graphs] `dtype` */
  const int32_t* n_edges_step; /* [1]: edges of the full list (above the capacity when it did not fit) */
  const void* virial_step;     /* xeq_npt_back alone: [9] `dtype`, the step's virial W = -dE/dstrain */
  const int32_t* reps_needed;  /* xeq_npt_back alone: [3], the images per axis the device's cell needs; NULL: no check */
  int64_t reps[3];             /* xeq_npt_back alone: the images per axis the graph was captured with */
} xeq_res_step;

/* The fixed-order per-graph sums.  chunk_atom0 / chunk_n [n_chunks] name at most XEQ_MD_CHUNK consecutive atoms of ONE graph, counted
 * from the graph's first atom; graph_chunk_ptr [n_graphs + 1] gives a graph's chunks.  The caller builds the three once from ptr. */
typedef struct xeq_res_chunks {
  const int32_t* chunk_atom0;
  const int32_t* chunk_n;
  const int32_t* graph_chunk_ptr;
  double* partial;      /* [n_chunks] (FIRE: [n_chunks, 4]; L-BFGS: [n_chunks, 3 (2 memory + 3) + 1]): the chunks' sums */
  int32_t* partial_bad; /* [n_chunks] (L-BFGS: [n_chunks, 4]): the chunks' non-finite-force flags */
} xeq_res_chunks;

/* The trajectory a back entry writes.  A NULL record, every = 0 or rows = 0: nothing is recorded.  When d = book[0] - start behind the
 * step (FIRE: book[0] read BEFORE the increment: this evaluation's number) is a positive multiple of `every`, row d / every - 1 (< rows)
 * is written; the MD backs record with `advance` alone. */
typedef struct xeq_res_recorder {
  int64_t every, start, rows;
  void* traj_pos;         /* [rows, n, 3] `dtype`, unwrapped: pos + image . cell (xeq_npt_back: by the current cell) */
  void* traj_epot;        /* [rows, n_graphs] `dtype` */
  void* traj_second;      /* [rows, n_graphs] `dtype`: the kinetic energy (dynamics), fmax (FIRE, L-BFGS) */
  int64_t* traj_step;     /* [rows] */
  void* traj_cell;        /* xeq_npt_back alone: [rows, 3, 3] `dtype` */
  double* traj_pressure;  /* xeq_npt_back alone: [rows], P p_unit */
} xeq_res_recorder;

/* Molecular dynamics (xequinet_amd/md.py).  Per-atom arithmetic runs in double whatever `dtype` is and is rounded
 * once where it is stored.
 *
 * Generator: Philox4x32-10 with key = (seed low word, seed high word) and counter
 *   c0 = rng_id low word, c1 = rng_id high word, c2 = step low word, c3 = step bits 32 .. 61 | purpose << 30
 * (purpose 0: the Langevin O step, 1: Maxwell-Boltzmann velocities; step < 2^62).  With u_k = (word_k + 1) 2^-32 in (0, 1], rounded once
 * to `dtype`: z0 = sqrt(-2 ln u_0) cos(2 pi u_1), z1 = sqrt(-2 ln u_0) sin(2 pi u_1), z2 = sqrt(-2 ln u_2) cos(2 pi u_3), with the accurate
 * logf / sincosf for f32 and log / sincos for f64.
 * xeq_md_normals: words [n, 4] (uint32, optional) and normals [n, 3] (`dtype`, optional) of the ids rng_id [n].
 *
 * xeq_md_front, per atom: [berendsen: v *= lambda_g, lambda_g = sqrt(1 + dt_over_tau (t0 / T_g - 1)) clamped to [0.9, 1.1] with
 * T_g = ke[g] tfac[g], and 1 where T_g is not positive]; v += dt / 2 * frc * inv_mass; [nve, berendsen: x += dt v] [langevin:
 * v' = c1 v + sqrt(noise2 inv_mass) z with z from (seed, 0, rng_id[i], book[0]); x += dt / 2 * (v + v'); v = v'];
 * then, with a cell and a periodic axis, the wrap: s = floor(x . inv(cell)) along the periodic axes, x -= s . cell, image [n, 3] += s
 * (applied twice: rounding to `dtype` can put an atom exactly on the far face).  dt = 0 is the wrap alone, whatever the ensemble (no
 * kick, no drift, no thermostat).
 *
 * xeq_md_back: the second half of a step.
 *   First launch, one workgroup per chunk: frc = frc_step; with `advance`, v += half_dt * frc * inv_mass; the chunk's kinetic energy
 *   sum_i half_mass_i |v_i|^2 in double (lanes, butterfly, the four waves in order) into partial [n_chunks]; its non-finite-force flag
 *   into partial_bad [n_chunks]; the recorder's positions.
 *   Second launch, one workgroup: ke[g] = the graph's partials in chunk order (one lane for up to four chunks, a wave with a butterfly
 *   beyond), epot[g] = energy_step[g]; then one lane: book[0] += advance, book[1] = max(book[1], n_edges_step[0]), book[2] = 1 on a
 *   non-finite force or energy.  With a single chunk the first launch's workgroup does this part itself and there is no second launch.
 *   No atomics; a graph's ke has the same bits alone and anywhere in a batch.
 * xeq_md_inverse_cell: the inverse the wrap uses (host only; inv [9] with frac_k = sum_j x_j inv[3 j + k]). */
#define XEQ_MD_CHUNK 256
enum { XEQ_MD_NVE = 0, XEQ_MD_LANGEVIN = 1, XEQ_MD_BERENDSEN = 2 };
enum { XEQ_MD_PURPOSE_LANGEVIN = 0, XEQ_MD_PURPOSE_MAXWELL = 1 };
typedef struct xeq_md_params {
  int64_t ensemble;        /* XEQ_MD_* (the barostat's entries run the Berendsen thermostat and do not read it) */
  const void* inv_mass;    /* [n] `dtype` = A / m_i (A: the factor from force / mass to length / fs^2; 0: a FIXED atom, which neither
                              moves nor keeps a velocity) */
  const void* half_mass;   /* [n] `dtype` = m_i / (2 A) (kinetic energy per squared velocity; 0 for a fixed atom) */
  void* ke;                /* [n_graphs] `dtype`: written by the back, read by the Berendsen thermostat */
  void* epot;              /* [n_graphs] `dtype` */
  const void* tfac;        /* [n_graphs] `dtype`: T_g = ke[g] tfac[g] */
  const int64_t* rng_id;   /* [n]: the atoms' generator ids (langevin) */
  uint64_t seed;
  double c1;               /* langevin: exp(-friction dt) */
  double noise2;           /* langevin: (1 - c1^2) k_B T */
  double dt_over_tau;      /* berendsen */
  double t0;               /* berendsen: the target temperature */
  double half_dt;          /* the back's kick */
} xeq_md_params;
int xeq_md_inverse_cell(const double* cell, double* inv);
int xeq_md_normals(int dtype, uint64_t seed, int purpose, uint64_t step, const int64_t* rng_id, int64_t n, uint32_t* words, void* normals,
                   void* stream);
int xeq_md_front(const xeq_res_system* sys, const xeq_md_params* md, double dt, void* stream);
int xeq_md_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                const xeq_res_recorder* rec, int advance, void* stream);

/* Constant pressure: the Berendsen barostat next to the Berendsen thermostat (ASE's NPTBerendsen.step in the front / back split above)
 * for ONE periodic box, all three axes periodic, whose cell lives on the device.  One step is xeq_npt_front, the step's graph (whose first
 * node forms the cell tables from the step's static cell: xeq_pbc_tables_device), xeq_npt_back.  Per-atom and per-box arithmetic runs in
 * double and is rounded once where it is stored.
 *
 * xeq_npt_back: everything xeq_md_back does for one graph; then the lane that keeps the books copies virial_step to virial and forms,
 * from the CURRENT cell c,
 *   V = |det c| (operation order of xeq_md_inverse_cell), P = (2 ke[0] + (W00 + W11) + W22) / (3 V) from the STORED ke[0],
 *   mu = 1 - kappa (p0 - P)   (ASE's linear form: no cube root, no clamp),
 *   pending cell = (dtype)(mu c) and its inverse.
 * A mu that is not finite or not positive, or a pending cell without an inverse, sets book[2] and leaves mu = 1, pending = current.
 * With reps_needed: book[3] = 1 when an entry exceeds reps; reps_seen keeps the largest seen.
 *
 * xeq_npt_front, dt > 0: the Berendsen lambda of xeq_md_front; x <- mu x for EVERY atom, fixed ones included (ASE's
 * set_cell(scale_atoms=True)); the half kick with the forces of the unscaled geometry and the drift for the free atoms; the wrap against
 * the PENDING cell.  Thread 0 alone commits the pending cell to the record's current cell and to step_cell; no other thread reads those
 * two in this launch.  dt = 0: the wrap against the current cell, nothing is committed.
 * So wherever the host can look, positions, images and step_cell belong together and mu is a function of the current state. */
#define XEQ_NPT_BOX 40
enum { XEQ_NPT_CELL = 0, XEQ_NPT_INV = 9, XEQ_NPT_CELL_NEXT = 18, XEQ_NPT_INV_NEXT = 27, XEQ_NPT_MU = 36, XEQ_NPT_P = 37, XEQ_NPT_V = 38 };
typedef struct xeq_npt_params {
  double* box;          /* the record, XEQ_NPT_BOX doubles: the current cell [9] (rows = lattice vectors; holds `dtype` values) and its
                           inverse [9] (frac_k = sum_j x_j inv[3 j + k]), the PENDING cell and its inverse, mu, P, V.  The host fills
                           current = pending = the start cell, the inverse by xeq_md_inverse_cell, mu = 1 */
  void* step_cell;      /* [9] `dtype`: the step's static cell */
  void* virial;         /* [9] `dtype`: the virial of the current positions and box */
  int32_t* reps_seen;   /* [3]: the largest reps_needed seen */
  double kappa;         /* (dt / taup) (beta / 3) */
  double p0;            /* the target pressure; energies per volume are in the caller's energy / length^3 */
  double p_unit;        /* converts P for the recorder alone */
} xeq_npt_params;
int xeq_npt_front(const xeq_res_system* sys, const xeq_md_params* md, const xeq_npt_params* npt, double dt, void* stream);
int xeq_npt_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                 const xeq_npt_params* npt, const xeq_res_recorder* rec, int advance, void* stream);

/* Canonical thermostats: a Nose-Hoover chain per graph (Martyna, Tuckerman, Tobias, Klein, Mol. Phys. 87, 1117 (1996)) and stochastic
 * velocity rescaling (Bussi, Donadio, Parrinello, J. Chem. Phys. 126, 014101 (2007)); DESIGN.md section 17.  Both are ONE factor s per
 * graph and step, a function of the graph's kinetic energy, so they ride on the two halves above: xeq_nvt_front is xeq_md_front's nve
 * step with the factor, xeq_nvt_back is xeq_md_back with the thermostat in its join.  The entries of xeq_md_params they read: inv_mass,
 * half_mass, ke, epot, seed, half_dt.  Every per-graph value is double whatever `dtype` is, in the order written here; exp, log, sqrt are
 * the double library functions.
 *
 * State: state [n_graphs, XEQ_NVT_ROW] doubles; a row holds the PENDING factor (XEQ_NVT_SCALE; the host starts it at 1), the thermostat's
 * energy term (XEQ_NVT_BATH; 0), and the chain's positions xi [8] and velocities vxi [8] (XEQ_NVT_XI, XEQ_NVT_VXI; 0).
 *
 * xeq_nvt_back: xeq_md_back, except that the lane that holds graph g's kinetic-energy sum K (the double, before it is rounded) runs, with
 * `advance`, one thermostat step for a whole `dt` and stores state[g][SCALE] = s and ke[g] = (dtype)((s s) K), which the recorder's row
 * takes too.  vel holds the velocities BEFORE the factor: it is pending until the next front.  With advance = 0, or Nf = 3 n_free[g] = 0,
 * or K not positive: s = 1 and the rest of the row is untouched; a step whose s is not finite and positive leaves s = 1 and the row
 * untouched too, and sets book[2] when s was not finite.  With nfkT = Nf kT, tau2 = tau tau, Q1 = nfkT tau2, Q = kT tau2 (Q_1 = Q1,
 * Q_k = Q beyond), M = chain_length:
 *
 *   XEQ_NVT_NOSE_HOOVER: s = 1; twice, with delta = dt / 2, hd = 0.5 delta, qd = 0.25 delta:
 *     for k = M .. 1:  G_1 = (2 K - nfkT) / Q1, G_k = (Q_{k-1} (vxi_{k-1} vxi_{k-1}) - kT) / Q;
 *                      k = M: vxi_M = vxi_M + hd G_M;  k < M: e = exp(-(qd vxi_{k+1})), vxi_k = vxi_k e, vxi_k = vxi_k + hd G_k,
 *                      vxi_k = vxi_k e;
 *     sigma = exp(-(delta vxi_1)), K = (sigma sigma) K, s = s sigma, xi_k = xi_k + delta vxi_k for every k;
 *     for k = 1 .. M: the same velocity update, every G from the values of that moment.
 *     bath = (sum_k 0.5 (Q_k (vxi_k vxi_k)), k rising, from 0) + nfkT xi_1 + kT (sum_{k >= 2} xi_k, k rising, from 0).
 *
 *   XEQ_NVT_BUSSI: c = exp(-(dt / tau)), q = ((1 - c) (0.5 nfkT)) / (Nf K), s2 = (c + q (R R + S)) + (2 R) sqrt(c q), s = sqrt(s2),
 *     bath = bath - (s2 - 1) K.  R is a standard normal, S a chi-square variate with Nf - 1 degrees of freedom, from the generator of
 *     xeq_md_normals under purpose XEQ_NVT_PURPOSE = 2 (xeq_md_normals itself serves purposes 0 and 1 alone): block j of the step is the
 *     block of (seed, 2, graph_rng_id[g] | j, book[0] before the increment); graph_rng_id [n_graphs] has a zero low word.  Of a block,
 *     z0 and z1 are the transform above evaluated in double and u = (word_2 + 1) 2^-32.  R = z0 of block 0.  Nf - 1 even: a = (Nf - 1) / 2,
 *     S = 2 Gamma(a); odd: a = (Nf - 2) / 2, S = 2 Gamma(a) + z1 z1 with z1 of block 0 (Nf is a multiple of 3: a >= 1).  Gamma(a) by
 *     Marsaglia and Tsang (ACM TOMS 26, 363 (2000)): d = a - 1 / 3, c' = 1 / sqrt(9 d); attempt j = 1, 2, ... takes x = z0 and u of block
 *     j, t = 1 + c' x, v = (t t) t, and is accepted when v > 0 and log(u) < ((0.5 (x x) + d) - d v) + d log(v); the result is d v.
 *     After XEQ_NVT_GAMMA_TRIES = 16 refused attempts the result is d |v| of the last one (probability below 1e-20).
 *
 * xeq_nvt_front, dt > 0: v = state[batch[i]][SCALE] v for every atom (double, where xeq_md_front applies the Berendsen lambda), then
 * xeq_md_front's nve step.  dt = 0: the wrap alone; the factor stays pending.  The front never writes the row. */
#define XEQ_NVT_ROW 18
#define XEQ_NVT_MAX_CHAIN 8
#define XEQ_NVT_GAMMA_TRIES 16
#define XEQ_NVT_PURPOSE 2
enum { XEQ_NVT_SCALE = 0, XEQ_NVT_BATH = 1, XEQ_NVT_XI = 2, XEQ_NVT_VXI = 10 };
enum { XEQ_NVT_NOSE_HOOVER = 0, XEQ_NVT_BUSSI = 1 };
/* Its record's number stands apart from the run 0 .. 8 above, which bindings walk as a dense table. */
enum { XEQ_REC_NVT = 16 };
struct xeq_nvt_params {
  int64_t kind;                /* XEQ_NVT_NOSE_HOOVER / XEQ_NVT_BUSSI */
  double* state;               /* [n_graphs, XEQ_NVT_ROW] */
  const int64_t* n_free;       /* [n_graphs]: the graph's free atoms; Nf = 3 n_free */
  const int64_t* graph_rng_id; /* [n_graphs] (bussi): the graphs' generator ids, low word zero */
  int64_t chain_length;        /* (nose-hoover) 1 .. XEQ_NVT_MAX_CHAIN */
  double kT;                   /* k_B T in the caller's energy unit, > 0 */
  double tau;                  /* the coupling time, > 0, in the unit of dt */
  double dt;                   /* the step the thermostat acts for */
};
typedef struct xeq_nvt_params xeq_nvt_params;
int xeq_nvt_front(const xeq_res_system* sys, const xeq_md_params* md, const xeq_nvt_params* nvt, double dt, void* stream);
int xeq_nvt_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_md_params* md,
                 const xeq_nvt_params* nvt, const xeq_res_recorder* rec, int advance, void* stream);

/* Batched geometry optimisation (FIRE; xequinet_amd/optimize.py).  Every graph is its own FIRE system.  Per-atom
 * and per-graph arithmetic runs in double whatever `dtype` is and is rounded once where it is stored.
 *
 * xeq_fire_back, behind evaluation number book[0]:
 *   First launch, one workgroup per chunk (chunk tables as for xeq_md_back): frc = frc_step (0 for a fixed atom; untouched for a converged
 *   graph); the chunk's P = sum f.v, ff = sum f.f, vv = sum v.v, max |f_i|^2 over its free atoms in double (lanes, butterfly, the four
 *   waves in order) into partial [n_chunks, 4]; its non-finite-force flag into partial_bad [n_chunks]; the recorder's positions.
 *   Second launch, one workgroup: a graph's partials in chunk order (one lane for up to four chunks, a wave with a butterfly beyond),
 *   then, by the lane that holds them, for a graph that is not converged: epot = energy_step, fmax = sqrt(max |f_i|^2);
 *     fmax < fmax_tol:  status = converged, converged_at = book[0]; nothing else, and nothing of this graph is written ever after;
 *     fresh:            c_v = 0, c_f = dt;
 *     P > 0:            c_v = 1 - alpha; if n_pos > n_min: dt = min(dt f_inc, dtmax), alpha *= f_alpha; n_pos += 1;
 *                       c_f = alpha_old sqrt(vv) / sqrt(ff) + dt;
 *     otherwise:        c_v = 0, alpha = alpha_start, dt *= f_dec, n_pos = 0, c_f = dt;
 *     then |v'|^2 = c_v^2 vv + 2 c_v c_f P + c_f^2 ff, norm = dt sqrt(|v'|^2), d = norm > maxstep ? dt (maxstep / norm) : dt,
 *     status = active.
 *   Then one lane: book[0] += 1, book[1] = max(book[1], n_edges_step[0]), book[2] = 1 on a non-finite force or energy of a graph that
 *   is not converged, book[3] = graphs not converged.  With a single chunk the first launch's workgroup does this part itself and
 *   there is no second launch.  No atomics; a graph's sums and state have the same bits alone and anywhere in a batch.
 * xeq_fire_front, per free atom of an ACTIVE graph: v = c_v v + c_f frc, x += d v, then the wrap of xeq_md_front.  Atoms of fresh or
 * converged graphs and fixed atoms are not written. */
enum { XEQ_FIRE_FRESH = 0, XEQ_FIRE_ACTIVE = 1, XEQ_FIRE_CONVERGED = 2 };
typedef struct xeq_fire_params {
  const uint8_t* fixed;    /* [n] or NULL; nonzero = the atom never moves, keeps v = 0, its force is left out of every sum and its entry
                              in frc is 0 */
  void* epot;              /* [n_graphs] `dtype` */
  void* fmax;              /* [n_graphs] `dtype` */
  double* dt;              /* [n_graphs] */
  double* alpha;           /* [n_graphs] */
  int32_t* n_pos;          /* [n_graphs]: evaluations with P > 0 in a row */
  int32_t* status;         /* [n_graphs]: XEQ_FIRE_FRESH (no velocity yet, ASE's `v is None`), _ACTIVE, _CONVERGED */
  int64_t* converged_at;   /* [n_graphs]: the evaluation at which the graph converged, counted from 0; the caller starts it at -1 */
  double* coef;            /* [n_graphs, 3] = (c_v, c_f, d) */
  double fmax_tol, maxstep, dtmax;
  int64_t n_min;
  double f_inc, f_dec, alpha_start, f_alpha;
} xeq_fire_params;
int xeq_fire_front(const xeq_res_system* sys, const xeq_fire_params* fire, void* stream);
int xeq_fire_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_fire_params* fire,
                  const xeq_res_recorder* rec, void* stream);

/* Batched limited-memory BFGS without line search (xequinet_amd/optimize.py: LBFGS, csrc/xeq_lbfgs.hip), by the rule
 * of ASE's optimize.LBFGS with use_line_search=False.  Every graph is its own minimiser: its own history, step clamp and convergence
 * flag.  The entries take the system, step, chunk and recorder records above and the driver's own state and parameters in
 * xeq_lbfgs_params.  Free atoms only: a fixed atom has force 0 and displacement 0 and enters no sum.  All per-graph and per-atom arithmetic
 * runs in double whatever `dtype` is and is rounded once where a `dtype` value is stored.  m = memory, K = 2 m + 1.
 *
 * State per graph: a ring of at most m pairs (s_j, y_j) in hist_s / hist_y, f64 [m, n, 3], slot j of a graph in its atoms' rows of
 * plane j; count and head of the ring (a pair goes to slot `head`, then head = (head + 1) mod m and count = min(count + 1, m), so the
 * filled slots are 0 .. count - 1 and the oldest pair is slot 0 until the ring is full, slot `head` from then on); status; converged_at;
 * epot; fmax; dropped; the symmetric Gram matrix gram [n_graphs, K, K] of the basis b = (s_0 .. s_{m-1}, y_0 .. y_{m-1}, g) by ring
 * slot (s_j at index j, y_j at m + j, g = -f at 2 m; entries of empty slots are not defined); delta [n_graphs, K], the direction's
 * coefficients (0 at empty slots).  sys->frc is f_prev between two backs; sys->vel is not used (NULL is taken).
 *
 * xeq_lbfgs_back, behind evaluation number book[0], for a graph that is not converged:
 *   1. f = frc_step, 0 for a fixed atom; epot = energy_step; fmax = sqrt(max_i |f_i|^2).
 *   2. fmax < fmax_tol: frc = f, status = converged, converged_at = book[0]; nothing of this graph is written ever after.
 *   3. otherwise, when the graph is ACTIVE, the candidate pair is s = pending_s (left by the front) and y = f_prev - f.
 *   4. The pair is stored at slot `head` only when s.y is finite and s.y > 0; a rejected pair leaves the history as it was and adds 1
 *      to dropped.
 *   5. frc = f (f_prev of the next back).
 *   6. The rows and columns of B that changed: the new pair's against everything stored and g's against everything.
 *   7. The two-loop recursion in coefficient space: delta = e_g; for the stored pairs from newest to oldest
 *      a_i = (B[s_i, :] . delta) / B[s_i, y_i], delta[y_i] -= a_i; delta *= 1 / alpha; for the pairs from oldest to newest
 *      beta = (B[y_i, :] . delta) / B[s_i, y_i], delta[s_i] += a_i - beta.  A fresh graph has delta = e_g (1 / alpha) and becomes ACTIVE.
 *   Orders.  First launch, one workgroup per chunk (chunk tables as for xeq_md_back): per atom the products (a0 b0 + a1 b1) + a2 b2 of
 *   the candidates s, y, g with every stored s_j, y_j and with one another, and |f_i|^2 for the max; lanes, butterfly, the four waves in
 *   order; into partial [n_chunks, 3 (2 m + 3) + 1] (candidate-major; columns: the s slots, the y slots, the candidates s, y, g; last
 *   the max).  partial_bad is int32 [n_chunks, 4] here: the chunk's non-finite-force flag and what the graph's status, head and count
 *   were in front of this back.  Second launch, one workgroup per chunk: a graph's partials are added chunk after chunk, sequentially,
 *   by every workgroup of the graph alike; each stores its atoms' rows of the ring and of frc; the workgroup of the graph's first chunk
 *   refreshes B and runs the recursion in one wave: lane l holds delta_l and delta_{64 + l}, a row product B[r, :] . delta is
 *   B[r, l] delta_l + B[r, 64 + l] delta_{64 + l} per lane (empty slots contribute 0) and a butterfly (xor 32, 16, .. 1).
 *   Every back, one lane (of the workgroup that ends last; it is elected by an integer ticket, which is 0 between launches and the only
 *   atomic -- no sum goes through it): a graph without atoms converges at its first evaluation; book[0] += 1, book[1] = max(book[1],
 *   n_edges_step[0]), book[2] = 1 on a non-finite force or energy of a graph that is not converged, book[3] = graphs not converged.
 *   No float atomics; a graph has the same bits alone and anywhere in a batch.
 * xeq_lbfgs_front, per free atom of an ACTIVE graph: p_i = -sum_k delta_k b_{k,i} in slot order (acc = 0; acc += delta_k b_k over the
 *   filled s slots, the filled y slots, then g = -(double)frc; p = -acc); longest = sqrt(max_i |p_i|^2) (chunk maxima: lanes,
 *   butterfly, waves; then over the graph's chunks); scale = maxstep / longest when longest >= maxstep, else 1;
 *   x_new = dtype(x + (damping scale) p_i); pending_s = (double)x_new - (double)x, exact, taken before the wrap; then the wrap of
 *   xeq_md_front.  Atoms of fresh or converged graphs and fixed atoms are not written.  First launch: direction (into pending_s) and
 *   chunk maxima (a chunk's first partial); second launch: the move.
 * max_graph_chunks: the most chunks any graph has; at most 1: the workgroup that owns a graph does both halves of an entry and each
 *   entry is ONE launch (a caller that understates it gets sums over a graph's own chunk alone, no access out of bounds).
 * The recorder's traj_second is fmax.  n = 0: the front does nothing; the back keeps the books.
 * Of the record, the front does not read gram, head, dropped, converged_at, epot, fmax, ticket, fmax_tol or alpha (they may be NULL / 0
 * there); the back does not read maxstep or damping. */
#define XEQ_LBFGS_MAX_MEMORY 32
enum { XEQ_LBFGS_FRESH = 0, XEQ_LBFGS_ACTIVE = 1, XEQ_LBFGS_CONVERGED = 2 };
typedef struct xeq_lbfgs_params {
  const uint8_t* fixed;       /* [n] or NULL; nonzero = the atom never moves, its force is left out of every sum and its entry in frc is 0 */
  double* hist_s;             /* [memory, n, 3]: the ring's s_j, plane j */
  double* hist_y;             /* [memory, n, 3]: the ring's y_j */
  double* pending_s;          /* [n, 3]: the direction between the front's two launches, the displacement s behind the front */
  double* gram;               /* [n_graphs, K, K]; the front does not read it */
  double* delta;              /* [n_graphs, K]: the direction's coefficients, written by the back, read by the front */
  int32_t* count;             /* [n_graphs]: pairs in the ring */
  int32_t* head;              /* [n_graphs]: the slot of the next pair; the front does not read it */
  int32_t* status;            /* [n_graphs]: XEQ_LBFGS_FRESH (no evaluation yet), _ACTIVE, _CONVERGED */
  int32_t* dropped;           /* [n_graphs]: rejected pairs; the front does not read it */
  int64_t* converged_at;      /* [n_graphs]: the evaluation at which the graph converged, counted from 0; the caller starts it at -1 */
  void* epot;                 /* [n_graphs] `dtype` */
  void* fmax;                 /* [n_graphs] `dtype` */
  int32_t* ticket;            /* [1]: the back's election, 0 between launches */
  int64_t memory;             /* m, 1 .. XEQ_LBFGS_MAX_MEMORY */
  int64_t max_graph_chunks;   /* the most chunks any graph has (above) */
  double fmax_tol, alpha;     /* read and checked by the back alone */
  double maxstep, damping;    /* read and checked by the front alone */
} xeq_lbfgs_params;
int xeq_lbfgs_front(const xeq_res_system* sys, const xeq_res_chunks* chunks, const xeq_lbfgs_params* lbfgs, void* stream);
int xeq_lbfgs_back(const xeq_res_system* sys, const xeq_res_step* step, const xeq_res_chunks* chunks, const xeq_lbfgs_params* lbfgs,
                   const xeq_res_recorder* rec, void* stream);

/* Batched harmonic analysis behind the Hessian front (xequinet_amd/vibrations.py, csrc/xeq_vib.hip).  Everything is
 * f64; only the Hessian is read as `dtype` and widened on load.  One workgroup per graph, fixed summation orders, no atomics: a graph's
 * result has the same bits alone and anywhere in a batch.  Graph g has n = ptr[g + 1] - ptr[g] atoms and m = 3 n coordinates.
 *
 * xeq_vib_project: hess holds the graphs' [n, n, 3, 3] blocks at the element offsets hess_off [n_graphs]; pos [N, 3]; mass [N] in amu.
 *   Writes per graph: mass_tot, moments [3] (ascending) and axes [9] (rows) of the inertia tensor about the centre of mass, rotor
 *   (XEQ_VIB_ATOM / _LINEAR: smallest moment <= 1e-6 x the largest / _NONLINEAR), n_tr (3 for an atom or with `periodic`, 5 linear, 6
 *   otherwise), q [6, m] at 18 ptr[g] (rows < n_tr: the orthonormal mass-weighted translations and rotations about the principal axes
 *   with a non-vanishing moment, modified Gram-Schmidt in that order), sigma = 2 |P S P|_F (1 when that is 0) and, at mat_off[g],
 *   M [m, m] = P S P + sigma Q Q^T with S = m^-1/2 (H + H^T)/2 m^-1/2, P = I - Q Q^T, formed through the rank-n_tr products.  work: scratch
 *   of q's shape.  With `periodic` no inertia tensor is formed (moments 0).  No size cap: it works in global memory.
 * xeq_vib_eigh: n symmetric matrices, matrix g of dimension dim[g] at mat_off[g]; eigenvalues ascending at val_off[g], eigenvectors
 *   [dim, dim] at mat_off[g] of `eigenvectors`, vector k contiguous, its largest-magnitude component (lowest index on a tie) positive;
 *   sweeps [n]; status [n]: 0, or 1 when XEQ_VIB_MAX_SWEEPS sweeps did not reach off(A) <= dim 2^-53 |A|_F.  Two-sided cyclic Jacobi in
 *   round-robin ordering, A and V in LDS sized from max_dim (>= every dim[g]); max_dim > XEQ_VIB_MAX_DIM is refused with
 *   XEQ_ERR_INVALID_ARGUMENT before any launch.
 * xeq_vib_eigh_large: the same arguments and the same output contract for dimensions up to XEQ_VIB_LARGE_MAX_DIM (any dim >= 1 is
 *   accepted, so the two entries can be compared on one matrix).  One workgroup per matrix working in the matrix's own block of
 *   `eigenvectors` in global memory (`mat` is only read; the two buffers must not overlap): Householder tridiagonalisation with
 *   accumulated Q, then implicit-shift QL with the rotations applied to Q^T.  sweeps: the largest number of QL iterations any one
 *   eigenvalue took; status 1 when one eigenvalue took more than XEQ_VIB_MAX_SWEEPS, or an eigenvalue is not finite.  max_dim >
 *   XEQ_VIB_LARGE_MAX_DIM is refused with XEQ_ERR_INVALID_ARGUMENT before any launch: 768 is 256 atoms, and above it one workgroup per
 *   matrix is the wrong shape for the work (a solver that spreads one matrix over the device is not built; vibrations.py keeps
 *   torch.linalg.eigh there).
 * xeq_vib_finish: from the lowest m - n_tr eigenpairs of graph g (eigenvalues at 3 ptr[g]), at mode_ptr[g] (norm_mode [k, n, 3] at
 *   mode_off[g]): eigenvalue, norm_mode = m_i^-1/2 v_k, reduced_mass = 1 / sum norm_mode^2, freq_wavenumber = sign(l) sqrt(|l|)
 *   to_wavenumber, vib_temperature = sign(l) sqrt(|l|) to_kelvin, force_const = reduced_mass l; n_imaginary [n_graphs].
 * xeq_vib_thermo_sums: sums [n_graphs, 4] over the modes with eigenvalue > 0, x = vib_temperature / temperature:
 *   theta / 2, theta / (e^x - 1), x / (e^x - 1) - ln(1 - e^-x), x^2 e^x / (e^x - 1)^2. */
#define XEQ_VIB_MAX_DIM 96
#define XEQ_VIB_LARGE_MAX_DIM 768
#define XEQ_VIB_MAX_SWEEPS 30
enum { XEQ_VIB_ATOM = 0, XEQ_VIB_LINEAR = 1, XEQ_VIB_NONLINEAR = 2 };
int xeq_vib_project(int dtype, const void* hess, const int64_t* hess_off, const double* pos, const double* mass, const int64_t* ptr,
                    int64_t n_graphs, int periodic, const int64_t* mat_off, double* mat, double* q, double* work, double* moments, double* axes,
                    double* mass_tot, int32_t* n_tr, int32_t* rotor, double* sigma, void* stream);
int xeq_vib_eigh(const double* mat, const int64_t* mat_off, const int64_t* val_off, const int32_t* dim, int64_t n, int max_dim,
                 double* eigenvalues, double* eigenvectors, int32_t* sweeps, int32_t* status, void* stream);
int xeq_vib_eigh_large(const double* mat, const int64_t* mat_off, const int64_t* val_off, const int32_t* dim, int64_t n, int max_dim,
                       double* eigenvalues, double* eigenvectors, int32_t* sweeps, int32_t* status, void* stream);
int xeq_vib_finish(const double* eigenvalues, const double* eigenvectors, const int64_t* mat_off, const double* mass, const int64_t* ptr,
                   int64_t n_graphs, const int32_t* n_tr, const int64_t* mode_ptr, const int64_t* mode_off, double to_wavenumber, double to_kelvin,
                   double* eigenvalue, double* norm_mode, double* reduced_mass, double* freq_wavenumber, double* vib_temperature,
                   double* force_const, int32_t* n_imaginary, void* stream);
int xeq_vib_thermo_sums(const double* vib_temperature, const double* eigenvalue, const int64_t* mode_ptr, int64_t n_graphs, double temperature,
                        double* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XEQ_H */
