// TorchScript-visible operators over the C ABI of libxeq_hip.so (include/xeq.h).
//
// Reference: the reference ships its models to LAMMPS / GROMACS as TorchScript files (run/jit_script.py:28-86 scripts
// interface/jit_model.py:12-216 and saves it with `_extra_files`); its hot ops live in third-party extensions that are
// themselves registered torch operators (torch_scatter, torch_cluster), so `torch.jit.script` sees schemas, not Python.
// This file gives the HIP path the same footing: operators in the `xeq::` namespace with schemas, registered through
// TORCH_LIBRARY, loadable from Python (`torch.ops.load_library`) and from a libtorch host program (dlopen before
// torch::jit::load).
//
//   xeq::xpainn_eval      ONE operator for a whole energy (+ forces, + virial) evaluation of XPaiNN (nn/model.py:26-46):
//                         edge geometry -> embedding -> n x [message + update] -> energy head -> explicit reverse pass.
//                         Every stage is the same HIP kernel the Python modules launch (nn/fused.py is the Python twin of
//                         this file and the two are compared bit for bit in tests/test_gpu_interface.py); the scalar MLPs
//                         are xeq_mlp2_fwd / _bwd, the o3.Linear contractions ATen GEMMs.  Enqueued from C++: a batch with a never-seen topology costs its
//                         GPU time plus ~150 native launches, no Python between kernels and no graph capture.
//                         Autograd: `energy` is differentiable w.r.t. `pos` (backward = -forces), which is how the
//                         GROMACS-style model hands forces to its caller (interface/jit_model.py:208-214).
//   xeq::radius_graph     open-boundary neighbour list (data/transform.py:58-64), canonical (center, neighbor) order.
//   xeq::radius_graph_pbc periodic single-system neighbour list with the reference's order and cell offsets
//                         (data/radius_graph.py:195-275 `single_radius_graph`, called inside the scripted GROMACS model,
//                         interface/jit_model.py:183-195).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <array>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <optional>
#include <unordered_map>
#include <vector>

#include "../../include/xeq.h"

namespace {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

#define XCALL(...)                                                                                  \
  do {                                                                                              \
    const int st_ = (__VA_ARGS__);                                                                  \
    TORCH_CHECK(st_ == 0, "xequinet_amd: ", #__VA_ARGS__, " failed (", st_, "): ", xeq_last_error()); \
  } while (0)

void* cur_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }
const float* PF(const Tensor& t) { return t.defined() ? (const float*)t.data_ptr() : nullptr; }   // f32 kernels; nullptr: absent
float* PFm(Tensor& t) { return t.defined() ? (float*)t.data_ptr() : nullptr; }
int dcode(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kDouble, "xequinet_amd: float32 / float64 tensors only");
  return t.scalar_type() == at::kFloat ? XEQ_F32 : XEQ_F64;
}
void need_hip(const Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), "xequinet_amd ops run on MI355X (HIP) tensors only and have no CPU fallback; ", what, " is on ", t.device());
}

// ---------------------------------------------------------------------------------------------- the packed-weight cache
// Every packed copy of a weight this file makes lives in ONE cache, `packed<Entry>` below (xequinet_amd/lib.py::cached is what the
// Python front uses).  An entry is rebuilt when a version counter, the pack epoch or an address of one of its tensors moves, and
// is valid only while the storage it was packed from is ALIVE (weak references): a freed parameter's address is
// reused by the allocator, typically by the next model's parameter of the same shape with the same version count.
// The references are to the STORAGE (not the tensor object): XPaiNNNative hands over fresh views of one flat parameter
// buffer on every call -- same storage, same address, shared version counter -- and those must hit the cache.
using WeakStore = c10::weak_intrusive_ptr<c10::StorageImpl>;
struct Owners {
  std::vector<std::optional<WeakStore>> refs;   // nullopt: an undefined tensor (absent bias)
  void set(std::initializer_list<const Tensor*> ts) {
    refs.clear();
    for (const Tensor* t : ts) {
      if (t->defined() && t->has_storage()) refs.emplace_back(t->storage().getWeakStorageImpl());
      else refs.emplace_back(std::nullopt);
    }
  }
  bool same(std::initializer_list<const Tensor*> ts) const {
    if (refs.size() != ts.size()) return false;
    size_t i = 0;
    for (const Tensor* t : ts) {
      const bool d = t->defined() && t->has_storage();
      if (d != refs[i].has_value()) return false;
      if (d) {
        auto sp = refs[i]->lock();
        if (!sp || sp.get() != t->storage().unsafeGetStorageImpl()) return false;
      }
      ++i;
    }
    return true;
  }
};
// The entry of (`slot_key`: the address of the site's leading weight, `form`: which form of the pack, for a site with several), made
// by `build(entry)` from `tensors` (an undefined tensor: an absent one).  One mutex and one map per Entry type; the key is formed
// here and nowhere else: (version counter + pack epoch, address) per tensor, on the stack (this runs once per launch site).
constexpr size_t PACK_MAX_TENSORS = 12;
template <class Entry, class Build>
Entry& packed(const void* slot_key, std::initializer_list<const Tensor*> tensors, int64_t form, Build&& build) {
  struct Slot {
    std::array<int64_t, 2 * PACK_MAX_TENSORS> key;
    Owners owners;
    Entry entry;
  };
  static std::mutex mu;
  static std::map<std::pair<const void*, int64_t>, Slot> cache;
  TORCH_INTERNAL_ASSERT(tensors.size() <= PACK_MAX_TENSORS);
  const int64_t epoch = (int64_t)xeq_pack_epoch() << 32;
  std::array<int64_t, 2 * PACK_MAX_TENSORS> key{};
  size_t n = 0;
  for (const Tensor* t : tensors) {
    key[n++] = t->defined() ? (int64_t)t->_version() + epoch : -1;
    key[n++] = t->defined() && t->numel() > 0 ? (int64_t)(intptr_t)t->data_ptr() : 0;
  }
  std::lock_guard<std::mutex> lock(mu);
  Slot& s = cache[{slot_key, form}];
  if (!s.owners.same(tensors) || s.key != key) {   // (a fresh slot has no owners: it misses)
    build(s.entry);
    s.owners.set(tensors);
    s.key = key;
  }
  return s.entry;
}

// ---------------------------------------------------------------------------------------------- two-layer MLPs
// Linear-SiLU-Linear on the matrix cores (hidden width 128: xeq_mlp2_fwd / _bwd, 32 .. 256: xeq_mlp2h_fwd / _bwd, csrc/xeq_mlp.hip)
// from fragment-order weight copies; Python: nn/fused.py::_mlp_packs / _mlp_fwd / _mlp_bwd.
constexpr int64_t MLP_H = 128;   // the hidden width of xeq_mlp2_fwd / _bwd / xeq_mlp2_and_linear
struct MlpPacks { Tensor w1p, w2p, w2tp, w1tp; };
const MlpPacks* mlp_packs(const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2) {
  if (w1.scalar_type() != at::kFloat || b1.numel() == 0 || b2.numel() == 0 ||
      !xeq_mlp2h_supported(XEQ_F32, (int)w1.size(1), (int)w1.size(0), (int)w2.size(0)))
    return nullptr;
  return &packed<MlpPacks>(w1.data_ptr(), {&w1, &b1, &w2, &b2}, 0, [&](MlpPacks& e) {
    const int h = (int)w1.size(0), k1 = (int)w1.size(1), n2 = (int)w2.size(0);
    const Tensor w1c = w1.detach().contiguous(), w2c = w2.detach().contiguous();
    auto pack = [&](const Tensor& w, const Tensor* bias, int n_out, int k_in, int transposed) {
      Tensor out = at::empty({xeq_mlp_packed_floats(n_out, k_in)}, w.options());
      XCALL(xeq_mlp_pack((const float*)w.data_ptr(), bias ? (const float*)bias->data_ptr() : nullptr, n_out, k_in, transposed,
                         (float*)out.data_ptr(), cur_stream()));
      return out;
    };
    e.w1p = pack(w1c, &b1, h, k1, 0);
    e.w2p = pack(w2c, &b2, n2, h, 0);
    e.w2tp = pack(w2c, nullptr, h, n2, 1);
    e.w1tp = pack(w1c, nullptr, k1, h, 1);
  });
}
// rbf_lin's rows in the wq message kernels' LDS layout (xeq_message_wq_pack_weights; Python: ops.wq_packed_weights): the kernels
// then stage a unit's weights with coalesced loads (XEQ_WQ_PACKED_WEIGHTS)
struct WqWeightPack { Tensor packed; };
const Tensor* wq_weight_pack(const Tensor& w, const Tensor& b, int num_basis, int node_dim, const int32_t mul[3]) {
  const int64_t n = xeq_message_wq_packed_weight_floats(num_basis, node_dim, mul);
  if (n <= 0 || w.scalar_type() != at::kFloat || !b.defined() || b.numel() == 0) return nullptr;
  return &packed<WqWeightPack>(w.data_ptr(), {&w, &b}, 0, [&](WqWeightPack& e) {
    const Tensor wc = w.detach().contiguous(), bc = b.detach().contiguous();
    e.packed = at::empty({n}, w.options());
    XCALL(xeq_message_wq_pack_weights(wc.data_ptr(), bc.data_ptr(), num_basis, node_dim, mul, e.packed.data_ptr(), cur_stream()));
  }).packed;
}
// x: [n, k1] rows with stride ldx (a column slice of a wider buffer is fine)
void mlp_fwd(const Tensor& x, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2, Tensor& pre, Tensor& y) {
  const MlpPacks* pk = (x.stride(1) == 1 && x.stride(0) % 4 == 0) ? mlp_packs(w1, b1, w2, b2) : nullptr;
  if (!pk) {
    pre = at::addmm(b1, x, w1.t());
    y = at::addmm(b2, at::silu(pre), w2.t());
    return;
  }
  const int64_t n = x.size(0);
  pre = at::empty({n, w1.size(0)}, x.options());
  y = at::empty({n, w2.size(0)}, x.options());
  if (w1.size(0) == MLP_H)
    XCALL(xeq_mlp2_fwd((const float*)x.data_ptr(), x.stride(0), n, (int)w1.size(1), (const float*)pk->w1p.data_ptr(),
                       (const float*)pk->w2p.data_ptr(), (int)w2.size(0), (float*)pre.data_ptr(), (float*)y.data_ptr(), w2.size(0), cur_stream()));
  else
    XCALL(xeq_mlp2h_fwd(XEQ_F32, (const float*)x.data_ptr(), x.stride(0), n, (int)w1.size(1), (int)w1.size(0), (const float*)pk->w1p.data_ptr(),
                        (const float*)pk->w2p.data_ptr(), (int)w2.size(0), (float*)pre.data_ptr(), (float*)y.data_ptr(), w2.size(0), cur_stream()));
}
Tensor mlp_bwd(const Tensor& g_y, const Tensor& pre, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2) {
  const MlpPacks* pk = mlp_packs(w1, b1, w2, b2);
  if (!pk) return at::mm(at::silu_backward(at::mm(g_y, w2), pre), w1);
  const Tensor g = g_y.contiguous();
  const int64_t n = g.size(0);
  Tensor g_x = at::empty({n, w1.size(1)}, g.options());
  if (w1.size(0) == MLP_H)
    XCALL(xeq_mlp2_bwd((const float*)g.data_ptr(), g.size(1), n, (int)g.size(1), (const float*)pk->w2tp.data_ptr(), (const float*)pre.data_ptr(),
                       (const float*)pk->w1tp.data_ptr(), (int)w1.size(1), (float*)g_x.data_ptr(), w1.size(1), cur_stream()));
  else
    XCALL(xeq_mlp2h_bwd(XEQ_F32, (const float*)g.data_ptr(), g.size(1), n, (int)g.size(1), (int)w1.size(0), (const float*)pk->w2tp.data_ptr(),
                        (const float*)pre.data_ptr(), (const float*)pk->w1tp.data_ptr(), (int)w1.size(1), (float*)g_x.data_ptr(), w1.size(1),
                        cur_stream()));
  return g_x;
}

// Single linear layers (dot_lin, the embedding, the head's first layer) through xeq_linear_fwd (csrc/xeq_linear.hip);
// Python: nn/fused.py::_linear_pack / _linear / linear_module_fwd / linear_module_bwd.
struct LinPack { Tensor fwd, bwd; };
const LinPack* lin_pack(const Tensor& w, const Tensor& b) {
  const int n_out = (int)w.size(0), k_in = (int)w.size(1);
  if (w.scalar_type() != at::kFloat || !xeq_linear_supported(XEQ_F32, k_in, n_out)) return nullptr;
  const bool has_bwd = xeq_linear_supported(XEQ_F32, n_out, k_in) != 0;   // (the embedding's 56 inputs: forward only, nobody differentiates it)
  const bool hb = b.defined() && b.numel() > 0;
  return &packed<LinPack>(w.data_ptr(), {&w, &b}, 0, [&](LinPack& e) {
    const Tensor wc = w.detach().contiguous();
    e.fwd = at::empty({xeq_mlp_packed_floats(n_out, k_in)}, w.options());
    XCALL(xeq_mlp_pack((const float*)wc.data_ptr(), hb ? (const float*)b.data_ptr() : nullptr, n_out, k_in, 0, (float*)e.fwd.data_ptr(), cur_stream()));
    e.bwd = Tensor();
    if (has_bwd) {
      e.bwd = at::empty({xeq_mlp_packed_floats(k_in, n_out)}, w.options());
      XCALL(xeq_mlp_pack((const float*)wc.data_ptr(), nullptr, k_in, n_out, 1, (float*)e.bwd.data_ptr(), cur_stream()));
    }
  });
}
// y = act(x W^T + b); row_index (int32, optional) gathers the rows of x; pre (optional) receives the pre-activation
Tensor linear_fwd(const Tensor& x, const Tensor& w, const Tensor& b, int act = 0, const Tensor* row_index = nullptr, Tensor* pre = nullptr) {
  const bool hb = b.defined() && b.numel() > 0;
  const LinPack* pk = (x.dim() == 2 && x.stride(1) == 1 && x.stride(0) % 4 == 0) ? lin_pack(w, b) : nullptr;
  if (!pk) {
    const Tensor xr = row_index ? x.index_select(0, row_index->to(at::kLong)) : x;
    Tensor y = hb ? at::addmm(b, xr, w.t()) : at::mm(xr, w.t());
    if (pre) *pre = y;
    return act == 1 ? at::silu(y) : y;
  }
  const int64_t n = row_index ? row_index->numel() : x.size(0);
  Tensor y = at::empty({n, w.size(0)}, x.options());
  if (pre) *pre = at::empty({n, w.size(0)}, x.options());
  XCALL(xeq_linear_fwd(x.data_ptr(), x.stride(0), n, (int)w.size(1), row_index ? (const int32_t*)row_index->data_ptr() : nullptr,
                       pk->fwd.data_ptr(), (int)w.size(0), hb, act, pre ? pre->data_ptr() : nullptr, y.data_ptr(), w.size(0), cur_stream()));
  return y;
}
Tensor linear_bwd(const Tensor& g_in, const Tensor& w, const Tensor& b) {   // dL/dx = g W
  const LinPack* pk = lin_pack(w, b);
  if (!pk || !pk->bwd.defined()) return at::mm(g_in, w);
  const Tensor g = g_in.contiguous();
  Tensor gx = at::empty({g.size(0), w.size(1)}, g.options());
  XCALL(xeq_linear_fwd(g.data_ptr(), g.stride(0), g.size(0), (int)w.size(0), nullptr, pk->bwd.data_ptr(), (int)w.size(1), 0, 0, nullptr,
                       gx.data_ptr(), w.size(1), cur_stream()));
  return gx;
}

// XPainnUpdate's two independent products side by side (xeq_mlp2_and_linear: one launch for MD-sized systems);
// Python: nn/fused.py::mlp_and_linear_fwd / _bwd.
void mlp_and_linear_fwd(const Tensor& x, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2, const Tensor& p, const Tensor& wl,
                        Tensor& pre, Tensor& y, Tensor& ip) {
  const MlpPacks* pk = (x.stride(1) == 1 && x.stride(0) % 4 == 0) ? mlp_packs(w1, b1, w2, b2) : nullptr;
  const LinPack* lp = (p.dim() == 2 && p.stride(1) == 1 && p.stride(0) % 4 == 0) ? lin_pack(wl, Tensor()) : nullptr;
  if (!pk || !lp || w1.size(0) != MLP_H) {   // (another hidden width: always the two launches, the MLP's first)
    mlp_fwd(x, w1, b1, w2, b2, pre, y);
    ip = linear_fwd(p, wl, Tensor());
    return;
  }
  const int64_t n = x.size(0);
  pre = at::empty({n, w1.size(0)}, x.options());
  y = at::empty({n, w2.size(0)}, x.options());
  ip = at::empty({n, wl.size(0)}, x.options());
  XCALL(xeq_mlp2_and_linear(0, (const float*)x.data_ptr(), x.stride(0), n, (int)w1.size(1), (const float*)pk->w1p.data_ptr(),
                            (const float*)pk->w2p.data_ptr(), (int)w2.size(0), (float*)pre.data_ptr(), (float*)y.data_ptr(), w2.size(0),
                            (const float*)p.data_ptr(), p.stride(0), (int)wl.size(1), (const float*)lp->fwd.data_ptr(), (int)wl.size(0),
                            (float*)ip.data_ptr(), wl.size(0), cur_stream()));
}
void mlp_and_linear_bwd(const Tensor& g_y, const Tensor& pre, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2,
                        const Tensor& g_lin_in, const Tensor& wl, Tensor& g_x, Tensor& g_p) {
  const MlpPacks* pk = mlp_packs(w1, b1, w2, b2);
  const LinPack* lp = lin_pack(wl, Tensor());
  if (!pk || !lp || !lp->bwd.defined() || w1.size(0) != MLP_H) {
    g_x = mlp_bwd(g_y, pre, w1, b1, w2, b2);
    g_p = linear_bwd(g_lin_in, wl, Tensor());
    return;
  }
  const Tensor g = g_y.contiguous(), gl = g_lin_in.contiguous();
  const int64_t n = g.size(0);
  g_x = at::empty({n, w1.size(1)}, g.options());
  g_p = at::empty({n, wl.size(1)}, g.options());
  XCALL(xeq_mlp2_and_linear(1, (const float*)g.data_ptr(), g.size(1), n, (int)g.size(1), (const float*)pk->w2tp.data_ptr(),
                            (const float*)pk->w1tp.data_ptr(), (int)w1.size(1), (float*)pre.data_ptr(), (float*)g_x.data_ptr(), w1.size(1),
                            (const float*)gl.data_ptr(), gl.stride(0), (int)wl.size(0), (const float*)lp->bwd.data_ptr(), (int)wl.size(1),
                            (float*)g_p.data_ptr(), wl.size(1), cur_stream()));
}

// [W_U | W_V] / sqrt(mul) blocks (prm layout: one [mul, 2 mul] tensor per l, empty when absent) in fragment order for
// xeq_update_uv_fwd / _bwd; Python: nn/fused.py::_packed_uv_frag.
struct UvFrag {
  Tensor w[3], wt[3];   // forward ([k_in = mul][n_out = 2 mul], biases folded) and reverse ([n_out = mul][k_in = 2 mul]) packs
};
constexpr int64_t UV_BWD_FUSE_NORM_MAX_NODES = 0;   // the constant of the same name in nn/fused.py, which says why
const UvFrag* uv_frag(const Tensor* q /* [W0, W1, W2, bias pair] */, int node_dim, const int32_t mul[3]) {
  if (q[0].scalar_type() != at::kFloat || !xeq_update_uv_supported(XEQ_F32, node_dim, mul)) return nullptr;
  int first = 0;
  while (first < 3 && mul[first] == 0) ++first;
  return &packed<UvFrag>(q[first].data_ptr(), {&q[0], &q[1], &q[2], &q[3]}, 0, [&](UvFrag& e) {
    for (int l = 0; l < 3; ++l) {
      e.w[l] = Tensor();
      e.wt[l] = Tensor();
      if (mul[l] == 0) continue;
      const Tensor W = q[l].detach().contiguous();   // [k_in = mul][n_out = 2 mul]
      e.w[l] = at::empty({xeq_mlp_packed_floats(2 * mul[l], mul[l])}, W.options());
      XCALL(xeq_mlp_pack((const float*)W.data_ptr(), (l == 0 && q[3].numel() > 0) ? (const float*)q[3].data_ptr() : nullptr, 2 * mul[l],
                         mul[l], 1, (float*)e.w[l].data_ptr(), cur_stream()));
      e.wt[l] = at::empty({xeq_mlp_packed_floats(mul[l], 2 * mul[l])}, W.options());
      XCALL(xeq_mlp_pack((const float*)W.data_ptr(), nullptr, mul[l], 2 * mul[l], 0, (float*)e.wt[l].data_ptr(), cur_stream()));
    }
  });
}

// ---------------------------------------------------------------------------------------------- fused node blocks
// One launch per direction for an update block and the front half of the message block behind it (csrc/xeq_nodeblock.hip;
// Python: nn/nodeblock.py::packed_fwd / packed_bwd / _uv_bias).  The packed weight programs are cached per update_mlp weight.
struct NbPacks { Tensor fwd, bwd, bias_uv; };
// q: the block's parameters (layout below), qn: the next block's (nullptr: no front half); gx: dL/dx_out is not zero
const NbPacks* nb_packs(const Tensor* q, const Tensor* qn, bool gx) {
  const bool tail = qn != nullptr;
  const Tensor none;
  return &packed<NbPacks>(q[15].data_ptr(), {&q[15], &q[10], &q[11], &q[12], &q[14], &q[17], &q[13], tail ? &qn[0] : &none, tail ? &qn[2] : &none},
                          (tail ? 2 : 0) + (gx ? 1 : 0), [&](NbPacks& e) {
    const auto bopt = q[15].options().dtype(at::kByte);
    const Tensor w3 = q[15].detach().contiguous(), dot = q[14].detach().contiguous(), w4 = q[17].detach().contiguous();
    const Tensor uv0 = q[10].contiguous(), uv1 = q[11].contiguous(), uv2 = q[12].contiguous();
    Tensor w1n, w2n;
    if (tail) {
      w1n = qn[0].detach().contiguous();
      w2n = qn[2].detach().contiguous();
    }
    e.fwd = at::empty({xeq_node_block_fwd_tiles(tail) * 3072}, bopt);
    XCALL(xeq_node_block_pack_fwd(PF(w3), PF(uv0), PF(uv1), PF(uv2), PF(dot), PF(w4), PF(w1n), PF(w2n), e.fwd.data_ptr(), cur_stream()));
    e.bwd = at::empty({xeq_node_block_bwd_tiles(tail, gx) * 3072}, bopt);
    XCALL(xeq_node_block_pack_bwd(PF(w3), PF(uv0), PF(uv1), PF(uv2), PF(dot), PF(w4), PF(w1n), PF(w2n), gx, e.bwd.data_ptr(), cur_stream()));
    e.bias_uv = q[13].numel() > 0 ? q[13].detach().contiguous() : Tensor();
  });
}

// ---------------------------------------------------------------------------------------------- graph plumbing
struct WqPlan {
  int n_ranges = 0;
  int64_t pcap = 0;
  Tensor qptr, pgath, peid, qinfo, sq, sn, win, rowptr, work, basis, dbasis;
  Tensor slot_rows, quad_rows;   // table form of the first block: element-table row per padded slot / per quad's owner (xeq_edge_basis_wq_table)
};
struct Graph {
  int64_t N = 0, E = 0;
  bool mirror = false;   // symmetric center-sorted list: the reverse wq kernel walks the forward plan (XEQ_WQ_MIRROR_WALK), ops.EdgeGraph.mirror_walk
  Tensor ei, c_rowptr, c_perm, n_rowptr, n_perm;   // c_perm undefined: edges already center-sorted.  n_*: the neighbor-sorted view (sorted_view)
  Tensor mirror_map;     // position of every edge's mirror edge (-1: none), for a list with `mirror`; an open list's is a permutation (= n_perm)
  WqPlan fwd, rev;
  Tensor table_z;        // the first block runs its table form: the atomic numbers its record launches index the element table by ...
  int64_t table_rows = 0;   // ... and the table's row count (ops.EdgeGraph.first_table)
  Tensor sb_basis, sb_dbasis;
  void sorted_view();    // builds n_rowptr / n_perm by a stable sort when nobody has yet (a periodic mirror map is not a permutation)
  // the edges by neighbor for a kernel that only sums over them (xeq_edge_vectors_bwd): the mirror map over the center rows, else the sorted view
  const Tensor& rev_rowptr() { if (!mirror_map.defined()) sorted_view(); return mirror_map.defined() ? c_rowptr : n_rowptr; }
  const Tensor& rev_perm() { if (!mirror_map.defined()) sorted_view(); return mirror_map.defined() ? mirror_map : n_perm; }
};

Tensor i32(int64_t n, const Tensor& like) { return at::empty({std::max<int64_t>(n, 1)}, like.options().dtype(at::kInt)); }

void csr_by_key(const Tensor& keys, int64_t n_rows, Tensor& rowptr, Tensor& perm) {
  const int64_t n = keys.numel(), bytes = xeq_csr_by_key_workspace(n, n_rows);
  TORCH_CHECK(bytes >= 0, "xequinet_amd: csr_by_key: sizes out of range");
  Tensor work = at::empty({std::max<int64_t>(bytes, 1)}, keys.options().dtype(at::kByte));
  rowptr = i32(n_rows + 1, keys);
  perm = i32(n, keys);
  XCALL(xeq_csr_by_key((const int64_t*)keys.data_ptr(), n, n_rows, work.data_ptr(), bytes, (int32_t*)rowptr.data_ptr(),
                       (int32_t*)perm.data_ptr(), cur_stream()));
}

void Graph::sorted_view() {
  if (!n_perm.defined()) csr_by_key(ei.select(0, 1), N, n_rowptr, n_perm);
}

// ops.EdgeGraph's twin.  symmetric && center_sorted: the promise of this package's list builders -- open boundaries: neighbours ascending
// and unique per center, (i, j) present iff (j, i) is; with cell_offsets (a periodic list): a center's edges ascending in (neighbor, image),
// (i, j, o) present iff (j, i, -o) is up to a rounding at the cutoff (include/xeq.h, xeq_reverse_edge_map_pbc).
Graph build_graph(const Tensor& edge_index, int64_t n_nodes, bool center_sorted, bool symmetric, const Tensor* cell_offsets) {
  Graph g;
  g.N = n_nodes;
  g.ei = edge_index.contiguous();
  g.E = g.ei.size(1);
  const Tensor center = g.ei.select(0, 0), nbr = g.ei.select(0, 1);
  if (center_sorted) {
    g.c_rowptr = i32(n_nodes + 1, g.ei);
    XCALL(xeq_csr_rowptr((const int64_t*)center.data_ptr(), g.E, n_nodes, (int32_t*)g.c_rowptr.data_ptr(), cur_stream()));
  } else {
    csr_by_key(center, n_nodes, g.c_rowptr, g.c_perm);
  }
  const char* env = std::getenv("XEQ_PBC_MIRROR");
  const bool periodic = cell_offsets != nullptr && cell_offsets->defined();
  g.mirror = symmetric && center_sorted && (!periodic || !(env && env[0] == '0' && env[1] == 0));
  if (g.mirror && !periodic) {
    g.n_rowptr = g.c_rowptr;
    g.n_perm = i32(g.E, g.ei);
    XCALL(xeq_reverse_edge_map((const int64_t*)g.ei.data_ptr(), g.E, n_nodes, (const int32_t*)g.c_rowptr.data_ptr(),
                               (int32_t*)g.n_perm.data_ptr(), cur_stream()));
    g.mirror_map = g.n_perm;
  } else if (g.mirror) {
    g.mirror_map = i32(g.E, g.ei);
    XCALL(xeq_reverse_edge_map_pbc(dcode(*cell_offsets), (const int64_t*)g.ei.data_ptr(), cell_offsets->data_ptr(), g.E, n_nodes,
                                   (const int32_t*)g.c_rowptr.data_ptr(), (int32_t*)g.mirror_map.data_ptr(), cur_stream()));
  } else {
    g.sorted_view();
  }
  return g;
}

void build_wq_plan(Graph& g, bool reverse, WqPlan& p) {
  if (reverse) g.sorted_view();
  const int eps = xeq_message_wq_edges_per_stream(g.N, g.E);   // (the C ABI states the rule; ops._wq_edges_per_stream asks it too)
  p.n_ranges = (int)std::max<int64_t>(1, (g.E + 2 * eps - 1) / (2 * eps));
  p.pcap = xeq_message_wq_pcap(g.N, g.E);
  p.qptr = i32(g.N + 1, g.ei);
  p.pgath = i32(p.pcap, g.ei);
  p.peid = i32(p.pcap, g.ei);
  p.qinfo = i32(p.pcap / 4, g.ei);
  p.sq = i32(2 * p.n_ranges + 1, g.ei);
  p.sn = i32(2 * p.n_ranges + 1, g.ei);
  p.win = i32(xeq_message_wq_win_ints(p.n_ranges), g.ei);
  const int64_t wbytes = xeq_message_wq_plan_workspace(g.N);
  TORCH_CHECK(wbytes >= 0, "xequinet_amd: wq plan workspace");
  p.work = at::empty({std::max<int64_t>(wbytes, 1)}, g.ei.options().dtype(at::kByte));
  p.rowptr = reverse ? g.n_rowptr : g.c_rowptr;
  const Tensor& perm = reverse ? g.n_perm : g.c_perm;
  const Tensor owner = g.ei.select(0, reverse ? 1 : 0), gather = g.ei.select(0, reverse ? 0 : 1);
  XCALL(xeq_message_wq_plan((const int32_t*)p.rowptr.data_ptr(), perm.defined() ? (const int32_t*)perm.data_ptr() : nullptr,
                            (const int64_t*)owner.data_ptr(), (const int64_t*)gather.data_ptr(), g.N, g.E, p.n_ranges,
                            p.work.data_ptr(), wbytes, (int32_t*)p.qptr.data_ptr(), (int32_t*)p.pgath.data_ptr(),
                            (int32_t*)p.peid.data_ptr(), (int32_t*)p.qinfo.data_ptr(), (int32_t*)p.sq.data_ptr(),
                            (int32_t*)p.sn.data_ptr(), (int32_t*)p.win.data_ptr(), cur_stream()));
}

// ---------------------------------------------------------------------------------------------- model description
// iparams: [node_dim, mul0, mul1, mul2, num_basis, n_blocks, rbf_kind, cutoff_kind, layer_norm, embed_kind(, charge_embed, spin_embed)]
//   (the last two only for a model with a charge / spin embedding: lists without them describe a model without either)
// fparams: [cutoff, invariant_eps]
// params (flat, in this order; undefined-by-absence entries are passed as empty tensors):
//   0 embed_table [87, A] (embed_kind 0) or embedding matrix [100, F] (embed_kind 1);  1 embed_w [F, A];  2 embed_b [F]
//   3 rbf_p0 [B];  4 rbf_p1 [B] (gaussian std; empty for bessel)
//   per block i (MSG = 5 + 27 i):
//     +0 mlp0_w [F,F]  +1 mlp0_b  +2 mlp2_w [H,F]  +3 mlp2_b  +4 rbf_w [H,B]  +5 rbf_b  +6 ln_w  +7 ln_b  +8 eq_w [C]  +9 eq_b [F]
//     +10 uv_pack_l0 [mul0, 2 mul0]  +11 uv_pack_l1  +12 uv_pack_l2  +13 uv_bias [2 F]
//     +14 dot_w [F, C]  +15 mlp3_w [F, F+C]  +16 mlp3_b  +17 mlp4_w [C+2F, F]  +18 mlp4_b  +19 ln_w  +20 ln_b  +21 eq_w  +22 eq_b
//     (+23..26 reserved)
//   tail: out0_w [Hd, F], out0_b, out2_w [1, Hd], out2_b
//   then, per electronic module present (charge first, then spin; nn/electronic.py): linear_q.weight [F, F], linear_q.bias [F],
//   linear_k.weight [F, 2|1], linear_v.weight [F, 2|1], residual.mlp.0.weight [F, F], residual.mlp.2.weight [F, F]
constexpr int P_BLOCK0 = 5, P_PER_BLOCK = 27, P_ELECTRONIC = 6;
struct Hyper {
  int F, mul[3], B, blocks, rbf_kind, cutoff_kind, layer_norm, embed_kind;
  double cutoff, inv_eps;
  int C() const { return mul[0] + mul[1] + mul[2]; }
  int D() const { return mul[0] + 3 * mul[1] + 5 * mul[2]; }
  int H() const { return F + 2 * C(); }
};

const Tensor* opt(const Tensor& t) { return t.defined() && t.numel() > 0 ? &t : nullptr; }
const void* OP(const Tensor& t) { return t.defined() && t.numel() > 0 ? t.data_ptr() : nullptr; }

// views of a BT buffer as plain matrices [n (2l+1), width * mul_l] per non-empty l  (nn/fused.py::_bt_blocks)
struct BtBlock {
  int l, m;
  Tensor view;
};
std::vector<BtBlock> bt_blocks(const Tensor& buf, int64_t n, const int mul[3], int width) {
  std::vector<BtBlock> out;
  int64_t base = 0;
  for (int l = 0; l < 3; ++l) {
    const int d = 2 * l + 1, m = mul[l];
    if (m > 0) out.push_back({l, m, buf.narrow(0, n * base * width, n * d * m * width).view({n * d, (int64_t)width * m})});
    base += (int64_t)d * m;
  }
  return out;
}

struct NormOut {
  Tensor shat, xhat, stats;
};
NormOut norm_fwd(const Hyper& hy, const Tensor& s, const Tensor& x, const Tensor& lw, const Tensor& lb, const Tensor& ew,
                 const Tensor& eb, Tensor shat_out, int64_t ld) {
  const int64_t n = x.size(0);
  NormOut o;
  if (!shat_out.defined()) {
    shat_out = at::empty({n, hy.F}, s.options());
    ld = hy.F;
  }
  o.shat = shat_out;
  o.xhat = at::empty({n * hy.D()}, x.options());
  o.stats = at::empty({n, 4}, s.options());
  XCALL(xeq_norm_fwd(dcode(s), s.data_ptr(), x.data_ptr(), hy.layer_norm ? lw.data_ptr() : nullptr,
                     hy.layer_norm ? lb.data_ptr() : nullptr, hy.layer_norm ? ew.data_ptr() : nullptr,
                     hy.layer_norm ? eb.data_ptr() : nullptr, n, hy.F, hy.mul, hy.layer_norm, o.shat.data_ptr(), ld,
                     o.xhat.data_ptr(), o.stats.data_ptr(), cur_stream()));
  return o;
}
// Front half of the FIRST message block from the element table (Python: nn/fused.py::first_block_front): behind the embedding a
// node's scalars are a function of its element and x = 0, so LayerNorm, EquivariantLayerNorm and scalar_mlp (nn/xpainn.py:128-139) are
// evaluated once per table row -- the same xeq_linear_fwd / xeq_norm_fwd / xeq_mlp2_fwd launches, which give a row the same bits in any
// batch -- and cached; an evaluation gathers (s, h, xhat's 0e block) by atomic number in ONE launch
// (xeq_first_block_front).  q: the first block's parameters.
struct ElementFront { Tensor rows_s, rows_h, rows_x0; };
const ElementFront* element_front(const Hyper& hy, const Tensor& table, const Tensor& ew, const Tensor& eb, const Tensor* q) {
  return &packed<ElementFront>(table.data_ptr(), {&table, &ew, &eb, &q[0], &q[1], &q[2], &q[3], &q[6], &q[7], &q[8], &q[9]}, 0, [&](ElementFront& e) {
    const int64_t zt = table.size(0);
    const Tensor z_all = at::arange(zt, table.options().dtype(at::kInt));
    e.rows_s = linear_fwd(table, ew, eb, 0, &z_all, nullptr);
    const Tensor x0 = at::zeros({zt, (int64_t)hy.D()}, table.options());
    NormOut no = norm_fwd(hy, e.rows_s, x0, q[6], q[7], q[8], q[9], Tensor(), 0);
    Tensor pre;
    mlp_fwd(no.shat, q[0], q[1], q[2], q[3], pre, e.rows_h);
    e.rows_h = e.rows_h.contiguous();
    e.rows_x0 = no.xhat.slice(0, 0, zt * hy.F).view({zt, (int64_t)hy.F}).contiguous();   // BT layout: the 0e block comes first
  });
}
void norm_bwd(const Hyper& hy, const Tensor& s, const Tensor& x, const Tensor& lw, const Tensor& ew, const Tensor& stats,
              const Tensor& g_shat, int64_t ld, const Tensor& g_xhat, const Tensor& res_s, const Tensor& res_x, Tensor& g_s,
              Tensor& g_x) {
  const int64_t n = x.size(0);
  g_s = at::empty_like(s);
  g_x = at::empty_like(x);
  XCALL(xeq_norm_bwd(dcode(s), s.data_ptr(), x.data_ptr(), hy.layer_norm ? lw.data_ptr() : nullptr,
                     hy.layer_norm ? ew.data_ptr() : nullptr, stats.data_ptr(), n, hy.F, hy.mul, hy.layer_norm, g_shat.data_ptr(), ld,
                     g_xhat.data_ptr(), res_s.defined() ? res_s.data_ptr() : nullptr, res_x.defined() ? res_x.data_ptr() : nullptr,
                     g_s.data_ptr(), g_x.data_ptr(), cur_stream()));
}

// The seed of an inference reverse pass behind the fused head: MINUS one (a [1] f32 constant, cached per device; nn/basic.py::_seed and
// nn/fused.py::constant_vector are its Python counterparts).  The reverse pass then returns -dE/dx = the forces without a negation launch -- and
// with the bits of the Python front: the bf16 matrix instructions are not symmetric in the sign (profiles/r05_mfma_sign.txt), so a pass
// seeded with +1 and negated afterwards differs in the last bit wherever a cotangent runs through the fused node block.  Not cached while
// a HIP graph is being captured (the tensor would live in that graph's pool).
Tensor minus_one(const at::TensorOptions& fopt) {
  static std::mutex mu;
  static std::unordered_map<int, Tensor> cache;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing((hipStream_t)cur_stream(), &capturing);
  std::lock_guard<std::mutex> lock(mu);
  const int dev = (int)fopt.device().index();
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  Tensor t = at::full({1}, -1.0, fopt.dtype(at::kFloat));
  if (capturing == hipStreamCaptureStatusNone) {
    (void)hipStreamSynchronize((hipStream_t)cur_stream());   // once: complete before any other stream may read it
    cache[dev] = t;
  }
  return t;
}

// ---------------------------------------------------------------------------------------------- the blocks of an evaluation
// One function per block and direction, named after its counterpart in nn/fused.py; xpainn_eval_impl below is their sequence.
// hy: the model, g: the edge list and its plans, q: the block's parameters (layout above), s / x: the node features, replaced by
// the block's outputs; g_s / g_x: their gradients, replaced likewise (an undefined g_x is zero).
struct MsgSaved {   // what a message block keeps for the reverse pass
  Tensor s, x, stats, pre, h, xhat;
  Tensor tab_z, tab_h, tab_x0;   // first block in its table form (nn/fused.py::first_block_table): atomic numbers, h_table, xhat0_table
};
struct UpdSaved {   // ... and an update block
  Tensor s, x, stats, uv, pre, a, ip;
};
struct EdgeGrad {   // dL/dvec over the blocks of the reverse pass (Python: ops.EdgeGradDeferral, same order: last block first)
  bool defer = false;             // wq: the blocks' partials are added up and the chain rule to dL/dvec runs ONCE, behind block 0
  std::vector<Tensor> part_sets;
  Tensor total;
};

// rbf_lin's rows for the wq kernels: the packed copy
const void* wq_weights(const Hyper& hy, const Tensor* q) {
  const Tensor* pk = wq_weight_pack(q[4], q[5], hy.B, hy.F, hy.mul);
  TORCH_CHECK(pk != nullptr, "xeq::xpainn_eval: rbf_lin weights cannot be packed for the wq kernels");
  return pk->data_ptr();
}

// XEmbedding.forward (nn/xpainn.py) and, where the table form covers the layout, nn/fused.py::first_block_front: the node scalars
// and the first block's norms and scalar_mlp in one gather by atomic number from per-element rows (m0.h is then defined).
// x: the zero equivariant features; wq: the wq message kernels follow; run_el: a charge / spin embedding follows.
Tensor embed_and_first_front(const Hyper& hy, const std::vector<Tensor>& prm, const Tensor& atomic_numbers, const Tensor& x, bool wq,
                             bool run_el, MsgSaved& m0) {
  const int64_t N = x.size(0);
  const int F = hy.F, D = hy.D(), H = hy.H();
  const auto fopt = x.options();
  const bool z_int = atomic_numbers.scalar_type() == at::kInt || atomic_numbers.scalar_type() == at::kLong;
  const bool table_form = hy.embed_kind == 0 && hy.blocks > 0 && x.scalar_type() == at::kFloat && hy.layer_norm && hy.mul[0] == F &&
                          prm[0].scalar_type() == at::kFloat && prm[0].dim() == 2 && prm[0].stride(1) == 1 && prm[0].stride(0) % 4 == 0 &&
                          lin_pack(prm[1], prm[2]) != nullptr;
  if (table_form && run_el) {
    // behind a charge / spin embedding the first block's scalars no longer depend on the element alone: the node scalars are gathered
    // from the per-element rows (nn/xpainn.py::XEmbedding.forward, ELEMENT_ROWS) and the first block takes its per-node launches
    const ElementFront* ef = element_front(hy, prm[0], prm[1], prm[2], &prm[P_BLOCK0]);
    return ef->rows_s.index_select(0, (z_int ? atomic_numbers : atomic_numbers.to(at::kLong)));
  }
  if (table_form) {
    const ElementFront* ef = element_front(hy, prm[0], prm[1], prm[2], &prm[P_BLOCK0]);
    const Tensor z = (z_int ? atomic_numbers : atomic_numbers.to(at::kLong)).contiguous();
    Tensor s = at::empty({N, (int64_t)F}, fopt);
    m0.h = at::empty({N, (int64_t)H}, fopt);
    m0.xhat = at::empty({N * (int64_t)D}, fopt);
    // the wq kernels' table form reads h and xhat from the table rows themselves (nn/fused.py::first_block_table): only s is gathered
    const bool table = xeq_message_wq_first_table(wq ? XEQ_FAMILY_WQ : XEQ_FAMILY_SB, ef->rows_h.size(0), 0, 0) != 0;
    // the wq kernels never read xhat's l > 0 blocks behind the embedding (XEQ_XHAT_HIGHER_L_ZERO): those are then not even written
    XCALL(xeq_first_block_front(z.data_ptr(), z.scalar_type() == at::kLong, N, ef->rows_s.size(0), ef->rows_s.data_ptr(),
                                ef->rows_h.data_ptr(), ef->rows_x0.data_ptr(), F, table ? 0 : H, table ? 0 : (wq ? F : D), s.data_ptr(),
                                m0.h.data_ptr(), m0.xhat.data_ptr(), cur_stream()));
    m0.s = s;
    m0.x = x;
    if (table) {
      m0.tab_z = z;
      m0.tab_h = ef->rows_h;
      m0.tab_x0 = ef->rows_x0;
    }
    return s;
  }
  if (hy.embed_kind == 0) {
    const Tensor z32 = atomic_numbers.to(at::kInt).contiguous();
    return linear_fwd(prm[0], prm[1], prm[2], 0, &z32);   // table lookup + Linear in one launch (nn/xpainn.py::XEmbedding._embed)
  }
  return prm[0].index_select(0, atomic_numbers.to(at::kLong));
}

// nn/electronic.py (csrc/xeq_electronic.hip): the charge, then the spin embedding, two launches each.  e: the first electronic
// parameter; has[kind]: the model has the module; total[kind]: the per-graph value, nullptr where the module does not run
Tensor electronic_fwd(const Hyper& hy, const Tensor* e, const bool has[2], const Tensor* const total_in[2], Tensor s, const Tensor& ptr64) {
  const int64_t N = s.size(0), G = ptr64.numel() - 1;
  for (int kind = 0; kind < 2; ++kind) {
    const Tensor* w = e;
    if (has[kind]) e += P_ELECTRONIC;
    if (!total_in[kind]) continue;
    const Tensor total = total_in[kind]->reshape({-1}).to(at::kFloat).contiguous();
    TORCH_CHECK(total.numel() == G, "xeq::xpainn_eval: ", kind == 0 ? "charge" : "spin", " has ", total.numel(), " values for ", G, " graphs");
    const LinPack* pq = lin_pack(w[0], w[1]);
    const LinPack* p1 = lin_pack(w[4], Tensor());
    const LinPack* p2 = lin_pack(w[5], Tensor());
    TORCH_CHECK(pq && p1 && p2, "xeq::xpainn_eval: the electronic module's weights cannot be packed");
    s = s.contiguous();
    Tensor attn = at::empty({N}, s.options()), s_out = at::empty({N, (int64_t)hy.F}, s.options());
    const Tensor wk = w[2].contiguous(), wv = w[3].contiguous();
    XCALL(xeq_electronic_fwd(kind, s.data_ptr(), s.stride(0), N, hy.F, (const int64_t*)ptr64.data_ptr(), G, total.data_ptr(),
                             pq->fwd.data_ptr(), wk.data_ptr(), wv.data_ptr(), p1->fwd.data_ptr(), p2->fwd.data_ptr(), attn.data_ptr(),
                             s_out.data_ptr(), cur_stream()));
    s = s_out;
  }
  return s;
}

// ops.message_forward's record launch: the radial / angular records of every edge for the message kernels.  wq (`wq`): along the
// forward plan, or the reverse one (`reverse`), with the derivative records when `want_d`; sb: value and derivative rows per edge
void edge_basis(const Hyper& hy, Graph& g, const Tensor& vec, const Tensor& p0, const Tensor& p1, bool wq, bool reverse, bool want_d) {
  const auto fopt = vec.options();
  if (wq) {
    WqPlan& w = reverse ? g.rev : g.fwd;
    build_wq_plan(g, reverse, w);
    w.basis = at::empty({w.pcap, xeq_message_wq_record_floats_for(hy.B)}, fopt);
    if (want_d) w.dbasis = at::empty({w.pcap, xeq_message_wq_record_floats_for(hy.B)}, fopt);
    if (g.table_z.defined()) {   // the first block's table form: the launch also writes the table rows of the plan's slots and quads
      w.slot_rows = i32(w.pcap, g.ei);
      w.quad_rows = i32(w.pcap / 4, g.ei);
      XCALL(xeq_edge_basis_wq_table(vec.data_ptr(), g.N, g.E, (const int32_t*)w.qptr.data_ptr(), (const int32_t*)w.peid.data_ptr(),
                                    hy.rbf_kind, hy.cutoff_kind, hy.B, hy.cutoff, p0.data_ptr(), OP(p1), w.basis.data_ptr(),
                                    w.dbasis.defined() ? w.dbasis.data_ptr() : nullptr, (const int32_t*)w.pgath.data_ptr(),
                                    (const int32_t*)w.qinfo.data_ptr(), g.table_z.data_ptr(), g.table_z.scalar_type() == at::kLong,
                                    g.table_rows, (int32_t*)w.slot_rows.data_ptr(), (int32_t*)w.quad_rows.data_ptr(), cur_stream()));
    } else {
      XCALL(xeq_edge_basis_wq(vec.data_ptr(), g.N, g.E, (const int32_t*)w.qptr.data_ptr(), (const int32_t*)w.peid.data_ptr(),
                              hy.rbf_kind, hy.cutoff_kind, hy.B, hy.cutoff, p0.data_ptr(), OP(p1), w.basis.data_ptr(),
                              w.dbasis.defined() ? w.dbasis.data_ptr() : nullptr, cur_stream()));
    }
  } else {
    const int w = xeq_edge_basis_width(hy.B);
    g.sb_basis = at::empty({g.E, w}, fopt);
    g.sb_dbasis = at::empty({g.E, w}, fopt);
    XCALL(xeq_edge_basis(dcode(vec), vec.data_ptr(), g.E, hy.rbf_kind, hy.cutoff_kind, hy.B, hy.cutoff, p0.data_ptr(), OP(p1),
                         g.sb_basis.data_ptr(), g.sb_dbasis.data_ptr(), cur_stream()));
  }
}

// The front half of fused.MessageBlock.forward (nn/xpainn.py:128-139): both norms and scalar_mlp, per node
void message_front_fwd(const Hyper& hy, const Tensor* q, const Tensor& s, const Tensor& x, MsgSaved& m) {
  m.s = s;
  m.x = x;
  NormOut no = norm_fwd(hy, s, x, q[6], q[7], q[8], q[9], Tensor(), 0);
  m.stats = no.stats;
  m.xhat = no.xhat;
  mlp_fwd(no.shat, q[0], q[1], q[2], q[3], m.pre, m.h);
}
// ... and of MessageBlock.backward: g_s / g_x arrive as the residual path's gradients
void message_front_bwd(const Hyper& hy, const Tensor* q, const MsgSaved& m, const Tensor& g_h, const Tensor& g_xhat, Tensor& g_s, Tensor& g_x) {
  const Tensor g_shat = mlp_bwd(g_h, m.pre, q[0], q[1], q[2], q[3]);
  Tensor ns, nx;
  norm_bwd(hy, m.s, m.x, q[6], q[8], m.stats, g_shat, hy.F, g_xhat, g_s, g_x, ns, nx);
  g_s = ns;
  g_x = nx;
}

// fused.MessageBlock.forward (nn/xpainn.py:128-161): the front half unless a gather or a fused node block has left it in m, then
// the message kernel.  first: the block behind the embedding (x = 0)
void message_block_fwd(const Hyper& hy, Graph& g, const Tensor* q, bool wq, bool first, MsgSaved& m, Tensor& s, Tensor& x) {
  if (!m.h.defined()) message_front_fwd(hy, q, s, x, m);
  Tensor s_out = at::empty_like(s), x_out = at::empty_like(x);
  if (wq && first && m.tab_h.defined()) {   // the table form: h and xhat from the element table's rows
    XCALL(xeq_message_fwd_wq_table(g.N, g.E, g.fwd.n_ranges, (const int32_t*)g.fwd.sq.data_ptr(), (const int32_t*)g.fwd.sn.data_ptr(),
                                   (const int32_t*)g.fwd.win.data_ptr(), (const int32_t*)g.fwd.rowptr.data_ptr(),
                                   (const int32_t*)g.fwd.slot_rows.data_ptr(), (const int32_t*)g.fwd.qinfo.data_ptr(), g.fwd.basis.data_ptr(),
                                   m.tab_h.data_ptr(), m.tab_x0.data_ptr(), m.tab_h.size(0), s.data_ptr(), x.data_ptr(), wq_weights(hy, q),
                                   nullptr, hy.B, hy.F, hy.mul, s_out.data_ptr(), x_out.data_ptr(),
                                   1 | XEQ_XHAT_HIGHER_L_ZERO | XEQ_WQ_PACKED_WEIGHTS, cur_stream()));
  } else if (wq) {
    XCALL(xeq_message_fwd_wq(g.N, g.E, g.fwd.n_ranges, (const int32_t*)g.fwd.sq.data_ptr(), (const int32_t*)g.fwd.sn.data_ptr(),
                             (const int32_t*)g.fwd.win.data_ptr(), (const int32_t*)g.fwd.rowptr.data_ptr(),
                             (const int32_t*)g.fwd.pgath.data_ptr(), (const int32_t*)g.fwd.qinfo.data_ptr(), g.fwd.basis.data_ptr(),
                             m.h.data_ptr(), m.xhat.data_ptr(), s.data_ptr(), x.data_ptr(), wq_weights(hy, q), nullptr, hy.B,
                             hy.F, hy.mul, s_out.data_ptr(), x_out.data_ptr(), (first ? (1 | XEQ_XHAT_HIGHER_L_ZERO) : 1) | XEQ_WQ_PACKED_WEIGHTS, cur_stream()));
  } else {
    XCALL(xeq_message_fwd_sb(dcode(s), g.N, g.E, (const int32_t*)g.c_rowptr.data_ptr(),
                             g.c_perm.defined() ? (const int32_t*)g.c_perm.data_ptr() : nullptr,
                             (const int64_t*)g.ei.select(0, 1).data_ptr(), g.sb_basis.data_ptr(), m.h.data_ptr(), m.xhat.data_ptr(),
                             s.data_ptr(), x.data_ptr(), q[4].data_ptr(), q[5].data_ptr(), hy.B, hy.F, hy.mul, s_out.data_ptr(),
                             x_out.data_ptr(), 1, cur_stream()));
  }
  s = s_out;
  x = x_out;
}

// fused.MessageBlock.backward without its front half: the message kernel's reverse; dL/dvec goes to eg.  g_h / g_xhat: the gradients
// of (h, xhat), undefined for the first block of a wq pass (only dL/dvec leaves it, the kernel then stores no node gradients)
void message_block_bwd(const Hyper& hy, Graph& g, const Tensor* q, bool wq, bool first, const Tensor& vec, const MsgSaved& m, const Tensor& g_s,
                       const Tensor& g_x, Tensor& g_h, Tensor& g_xhat, EdgeGrad& eg) {
  const int64_t N = g.N, E = g.E;
  void* st = cur_stream();
  const bool node_grads = !first || !wq;
  g_h = node_grads ? at::empty_like(m.h) : Tensor();
  g_xhat = node_grads ? at::empty_like(m.xhat) : Tensor();
  Tensor g_vec = at::empty_like(vec);
  if (wq) {
    Tensor parts = at::empty({std::max<int64_t>(1, xeq_message_wq_parts_floats(N, E, hy.mul))}, vec.options());
    const WqPlan& w = g.mirror ? g.fwd : g.rev;
    const int xl_bwd = (first ? (1 | XEQ_XHAT_HIGHER_L_ZERO) : 1) | (g.mirror ? XEQ_WQ_MIRROR_WALK : 0);
    if (first && m.tab_h.defined())
      XCALL(xeq_message_bwd_wq_table(N, E, w.n_ranges, (const int32_t*)w.sq.data_ptr(), (const int32_t*)w.sn.data_ptr(),
                                     (const int32_t*)w.win.data_ptr(), (const int32_t*)w.rowptr.data_ptr(),
                                     (const int32_t*)w.pgath.data_ptr(), (const int32_t*)w.qinfo.data_ptr(),
                                     (const int32_t*)w.quad_rows.data_ptr(), w.basis.data_ptr(), w.dbasis.data_ptr(), m.tab_h.data_ptr(),
                                     m.tab_x0.data_ptr(), m.tab_h.size(0), g_s.data_ptr(), g_x.data_ptr(), wq_weights(hy, q), nullptr, hy.B,
                                     hy.F, hy.mul, parts.data_ptr(), xl_bwd | XEQ_WQ_PACKED_WEIGHTS, st));
    else
    XCALL(xeq_message_bwd_wq(N, E, w.n_ranges, (const int32_t*)w.sq.data_ptr(), (const int32_t*)w.sn.data_ptr(),
                             (const int32_t*)w.win.data_ptr(), (const int32_t*)w.rowptr.data_ptr(),
                             (const int32_t*)w.pgath.data_ptr(), (const int32_t*)w.qinfo.data_ptr(),
                             w.basis.data_ptr(), w.dbasis.data_ptr(), m.h.data_ptr(), m.xhat.data_ptr(), g_s.data_ptr(),
                             g_x.data_ptr(), wq_weights(hy, q), nullptr, hy.B, hy.F, hy.mul, node_grads ? g_h.data_ptr() : nullptr,
                             node_grads ? g_xhat.data_ptr() : nullptr, parts.data_ptr(), xl_bwd | XEQ_WQ_PACKED_WEIGHTS, st));
    const int32_t* mirror_map = g.mirror ? (const int32_t*)g.mirror_map.data_ptr() : nullptr;
    if (eg.defer) {
      eg.part_sets.push_back(parts);
      if (first) {
        std::vector<const void*> pp;
        for (const Tensor& ps : eg.part_sets) pp.push_back(ps.data_ptr());
        XCALL(xeq_message_wq_edge_grad_sum(vec.data_ptr(), N, E, (const int32_t*)w.qptr.data_ptr(), (const int32_t*)w.peid.data_ptr(),
                                           mirror_map, hy.mul, (int)pp.size(), pp.data(), g_vec.data_ptr(), st));
        eg.total = g_vec;
      }
    } else {
      XCALL(xeq_message_wq_edge_grad(vec.data_ptr(), N, E, (const int32_t*)w.qptr.data_ptr(), (const int32_t*)w.peid.data_ptr(),
                                     mirror_map, hy.mul, parts.data_ptr(), g_vec.data_ptr(), st));
      eg.total = eg.total.defined() ? eg.total + g_vec : g_vec;
    }
  } else {
    g.sorted_view();
    // the blocks share ONE dL/dvec buffer: the first to run stores, the others add (XEQ_SB_ACCUM_VEC; ops.message_backward does the same)
    const bool accum = eg.total.defined();
    if (!accum) eg.total = g_vec;
    XCALL(xeq_message_bwd_sb(dcode(vec), N, E, (const int32_t*)g.n_rowptr.data_ptr(), (const int32_t*)g.n_perm.data_ptr(),
                             (const int64_t*)g.ei.select(0, 0).data_ptr(), g.sb_basis.data_ptr(), g.sb_dbasis.data_ptr(),
                             m.h.data_ptr(), m.xhat.data_ptr(), g_s.data_ptr(), g_x.data_ptr(), q[4].data_ptr(), q[5].data_ptr(),
                             hy.B, hy.F, hy.mul, g_h.data_ptr(), g_xhat.data_ptr(), eg.total.data_ptr(), 1 | (accum ? XEQ_SB_ACCUM_VEC : 0), st));
  }
}

// fused.NodeBlock.forward (nn/nodeblock.py::node_block_fwd): the update block and, with the next block's parameters qn, the front
// half of the message block behind it (saved in *mn) in one launch
void node_block_fwd(const Hyper& hy, const Tensor* q, const Tensor* qn, UpdSaved& u, MsgSaved* mn, Tensor& s, Tensor& x) {
  const int64_t N = s.size(0);
  const int F = hy.F, C = hy.C(), D = hy.D(), H = hy.H();
  const auto fopt = s.options();
  u.s = s;
  u.x = x;
  const NbPacks* pk = nb_packs(q, qn, qn != nullptr);
  const int64_t NR = xeq_node_block_rows(N);   // internal tensors: whole workgroups, wave-native layout
  u.uv = at::empty({2 * NR * D}, fopt);
  u.stats = at::empty({N, 4}, fopt);
  u.pre = at::empty({NR, F}, fopt);
  u.a = at::empty({NR, C + 2 * F}, fopt);
  u.ip = at::empty({NR, F}, fopt);
  Tensor p_scr = at::empty({NR, C}, fopt);
  Tensor s_out = at::empty_like(s), x_out = qn ? at::empty_like(x) : Tensor();
  if (mn) {
    mn->stats = at::empty({N, 4}, fopt);
    mn->xhat = at::empty({N * D}, fopt);
    mn->pre = at::empty({NR, F}, fopt);
    mn->h = at::empty({N, H}, fopt);
  }
  XCALL(xeq_node_block_fwd(N, PF(s), PF(x), PF(q[19]), PF(q[20]), PF(q[21]), PF(q[22]), PF(pk->bias_uv), PF(q[16]), PF(q[18]),
                           hy.inv_eps, pk->fwd.data_ptr(), PFm(p_scr), PFm(u.uv), PFm(u.stats), PFm(u.pre), PFm(u.a), PFm(u.ip),
                           PFm(s_out), PFm(x_out), qn ? PF(qn[6]) : nullptr, qn ? PF(qn[7]) : nullptr, qn ? PF(qn[8]) : nullptr,
                           qn ? PF(qn[9]) : nullptr, qn ? PF(qn[1]) : nullptr, qn ? PF(qn[3]) : nullptr,
                           mn ? PFm(mn->stats) : nullptr, mn ? PFm(mn->xhat) : nullptr, mn ? PFm(mn->pre) : nullptr,
                           mn ? PFm(mn->h) : nullptr, cur_stream()));
  s = s_out;
  x = x_out;
  if (mn) {
    mn->s = s;
    mn->x = x;
  }
}

// fused.NodeBlock.backward (nn/nodeblock.py::node_block_bwd).  pend_gh / pend_gxhat: the gradients of the next block's (h, xhat)
void node_block_bwd(const Hyper& hy, const Tensor* q, const Tensor* qn, const UpdSaved& u, const MsgSaved* mn, const Tensor& pend_gh,
                    const Tensor& pend_gxhat, Tensor& g_s, Tensor& g_x) {
  const int64_t N = u.s.size(0);
  const int C = hy.C(), D = hy.D();
  const auto fopt = u.s.options();
  const bool last_blk = qn == nullptr;
  const NbPacks* pk = nb_packs(q, qn, !last_blk);
  Tensor ns = at::empty_like(u.s), nx = at::empty_like(u.x);
  const int64_t NR = xeq_node_block_rows(N);
  Tensor gxo = last_blk ? Tensor() : at::empty({NR, D}, fopt);
  Tensor gp = at::empty({NR, C}, fopt), gv = at::empty({NR, C}, fopt), gw = at::empty({NR, D}, fopt);
  if (!last_blk && !g_x.defined()) g_x = at::zeros({N, D}, fopt);
  XCALL(xeq_node_block_bwd(N, PF(pend_gh), PF(pend_gxhat), PF(g_s), PF(g_x), mn ? PF(mn->s) : nullptr, mn ? PF(mn->x) : nullptr,
                           mn ? PF(mn->stats) : nullptr, mn ? PF(mn->pre) : nullptr, qn ? PF(qn[6]) : nullptr,
                           qn ? PF(qn[8]) : nullptr, PF(u.uv), PF(u.a), PF(u.ip), PF(u.pre), PF(u.s), PF(u.x), PF(u.stats), PF(q[19]),
                           PF(q[21]), hy.inv_eps, pk->bwd.data_ptr(), PFm(gxo), PFm(gp), PFm(gv), PFm(gw), PFm(ns), PFm(nx), cur_stream()));
  g_s = ns;
  g_x = nx;
}

// fused.UpdateBlock.forward (nn/xpainn.py:206-231).  last: the energy head reads the scalars only, the last equivariant output has
// no consumer
void update_block_fwd(const Hyper& hy, const Tensor* q, bool last, UpdSaved& u, Tensor& s, Tensor& x) {
  const int64_t N = s.size(0);
  const int F = hy.F, C = hy.C(), D = hy.D(), dt = dcode(s);
  const auto fopt = s.options();
  void* st = cur_stream();
  u.s = s;
  u.x = x;
  Tensor cat = at::empty({N, F + C}, fopt);
  u.uv = at::empty({2 * N * D}, fopt);
  Tensor p = at::empty({N, C}, fopt);
  if (const UvFrag* fr = uv_frag(&q[10], F, hy.mul)) {   // norms -> U, V -> v, p in one matrix-core launch
    u.stats = at::empty({N, 4}, fopt);
    XCALL(xeq_update_uv_fwd((const float*)s.data_ptr(), (const float*)x.data_ptr(), hy.layer_norm ? PF(q[19]) : nullptr,
                            hy.layer_norm ? PF(q[20]) : nullptr, hy.layer_norm ? PF(q[21]) : nullptr,
                            hy.layer_norm ? PF(q[22]) : nullptr, N, F, hy.mul, hy.layer_norm, PF(fr->w[0]), PF(fr->w[1]), PF(fr->w[2]),
                            q[13].numel() > 0, hy.inv_eps, (float*)cat.data_ptr(), F + C, (float*)p.data_ptr(),
                            (float*)u.uv.data_ptr(), (float*)u.stats.data_ptr(), st));
  } else {
    NormOut no = norm_fwd(hy, s, x, q[19], q[20], q[21], q[22], cat, F + C);
    u.stats = no.stats;
    auto xb = bt_blocks(no.xhat, N, hy.mul, 1), ub = bt_blocks(u.uv, N, hy.mul, 2);
    for (size_t k = 0; k < xb.size(); ++k) {
      const Tensor& W = q[10 + xb[k].l];
      if (xb[k].l == 0 && q[13].numel() > 0) at::addmm_out(ub[k].view, q[13], xb[k].view, W);
      else at::mm_out(ub[k].view, xb[k].view, W);
    }
    XCALL(xeq_uv_reduce_fwd(dt, u.uv.data_ptr(), N, hy.mul, hy.inv_eps, cat.data_ptr(), F + C, F, p.data_ptr(), st));
  }
  mlp_and_linear_fwd(cat, q[15], q[16], q[17], q[18], p, q[14], u.pre, u.a, u.ip);
  Tensor s_out = at::empty_like(s), x_out = last ? Tensor() : at::empty_like(x);
  XCALL(xeq_update_out_fwd(dt, s.data_ptr(), x.data_ptr(), u.uv.data_ptr(), u.a.data_ptr(), u.ip.data_ptr(), N, F, hy.mul,
                           s_out.data_ptr(), last ? nullptr : x_out.data_ptr(), st));
  s = s_out;
  x = x_out;
}

// fused.UpdateBlock.backward
void update_block_bwd(const Hyper& hy, const Tensor* q, const UpdSaved& u, Tensor& g_s, Tensor& g_x) {
  const int64_t N = u.s.size(0);
  const int F = hy.F, C = hy.C(), D = hy.D(), dt = dcode(u.s);
  const auto fopt = u.s.options();
  void* st = cur_stream();
  Tensor g_a = at::empty_like(u.a), g_ip = at::empty_like(u.ip);
  const void* gx_ptr = g_x.defined() ? g_x.data_ptr() : nullptr;
  XCALL(xeq_update_out_bwd(dt, g_s.data_ptr(), gx_ptr, u.uv.data_ptr(), u.a.data_ptr(), u.ip.data_ptr(), N, F, hy.mul,
                           g_a.data_ptr(), g_ip.data_ptr(), nullptr, st));
  Tensor g_p, g_cat;
  mlp_and_linear_bwd(g_a, u.pre, q[15], q[16], q[17], q[18], g_ip, q[14], g_cat, g_p);
  Tensor ns, nx;
  const UvFrag* fr = g_cat.is_contiguous() ? uv_frag(&q[10], F, hy.mul) : nullptr;
  if (fr) {   // dL/dU, dL/dV -> dL/dxhat (-> reverse of both norms) in one matrix-core launch
    const bool fuse = N <= UV_BWD_FUSE_NORM_MAX_NODES;
    Tensor g_xhat;
    if (fuse) {
      ns = at::empty_like(u.s);
      nx = at::empty_like(u.x);
    } else {
      g_xhat = at::empty({N * D}, fopt);
    }
    XCALL(xeq_update_uv_bwd((const float*)u.uv.data_ptr(), (const float*)g_p.data_ptr(), (const float*)g_cat.data_ptr(), F + C,
                            (const float*)gx_ptr, (const float*)g_s.data_ptr(), (const float*)u.a.data_ptr(), u.a.size(1),
                            (const float*)u.s.data_ptr(), (const float*)u.x.data_ptr(), (const float*)u.stats.data_ptr(),
                            hy.layer_norm ? PF(q[19]) : nullptr, hy.layer_norm ? PF(q[21]) : nullptr, N, F, hy.mul, hy.layer_norm,
                            PF(fr->wt[0]), PF(fr->wt[1]), PF(fr->wt[2]), hy.inv_eps, fuse ? (float*)ns.data_ptr() : nullptr,
                            fuse ? (float*)nx.data_ptr() : nullptr, fuse ? nullptr : (float*)g_xhat.data_ptr(), st));
    if (!fuse) norm_bwd(hy, u.s, u.x, q[19], q[21], u.stats, g_cat, F + C, g_xhat, g_s, g_x, ns, nx);
  } else {
    Tensor g_uv = at::empty_like(u.uv);
    if (!g_x.defined()) g_x = at::zeros({N, D}, fopt);   // the kernel chain wants the tensor
    XCALL(xeq_uv_reduce_bwd(dt, u.uv.data_ptr(), g_p.data_ptr(), g_cat.data_ptr(), F + C, F, N, hy.mul, hy.inv_eps, g_x.data_ptr(),
                            u.a.data_ptr(), g_uv.data_ptr(), st));
    Tensor g_xhat = at::empty({N * D}, fopt);
    auto gb = bt_blocks(g_xhat, N, hy.mul, 1), gub = bt_blocks(g_uv, N, hy.mul, 2);
    for (size_t k = 0; k < gb.size(); ++k) at::mm_out(gb[k].view, gub[k].view, q[10 + gb[k].l].t());
    norm_bwd(hy, u.s, u.x, q[19], q[21], u.stats, g_cat, F + C, g_xhat, g_s, g_x, ns, nx);
  }
  g_s = ns;
  g_x = nx;
}

// EnergyOut.forward (nn/output.py:114-128) in the three forms of the Python front: fused.EnergyReadout (the head with its whole
// reverse pass saved as one row per node, ONE launch), fused.EnergyHead (the same kernels layer by layer), else the library GEMMs.
// t: the head's parameters
struct HeadSaved {
  const LinPack* pk = nullptr;
  bool native = false, fused = false;
  Tensor pre_o, jac;
};
void energy_readout_fwd(const Hyper& hy, const Tensor* t, const Tensor& s, const Tensor& ptr64, bool want_bwd, HeadSaved& hd, Tensor& atomic,
                        Tensor& energy) {
  const int64_t N = s.size(0), G = ptr64.numel() - 1;
  const int F = hy.F, dt = dcode(s);
  const auto fopt = s.options();
  void* st = cur_stream();
  hd.pk = dt == XEQ_F32 && t[0].size(0) % 4 == 0 && t[2].size(0) == 1 ? lin_pack(t[0], t[1]) : nullptr;
  hd.native = hd.pk != nullptr && hd.pk->bwd.defined();
  hd.fused = hd.native && s.stride(1) == 1 && s.stride(0) % 4 == 0 && t[1].defined() && t[1].numel() > 0 &&
             xeq_head_supported(XEQ_F32, F, (int)t[0].size(0));
  if (hd.fused) {
    atomic = at::empty({N}, fopt);
    if (want_bwd) hd.jac = at::empty({N, (int64_t)F}, fopt);
    XCALL(xeq_head_fwd(s.data_ptr(), s.stride(0), N, F, (int)t[0].size(0), hd.pk->fwd.data_ptr(), hd.pk->bwd.data_ptr(), t[2].data_ptr(),
                       t[3].data_ptr(), atomic.data_ptr(), hd.jac.defined() ? hd.jac.data_ptr() : nullptr, st));
  } else if (hd.native) {
    const Tensor hidden = linear_fwd(s, t[0], t[1], 1, nullptr, &hd.pre_o);
    atomic = at::empty({N}, fopt);
    XCALL(xeq_head_dot(hidden.data_ptr(), N, (int)t[0].size(0), t[2].data_ptr(), t[3].data_ptr(), atomic.data_ptr(), st));
  } else {
    hd.pre_o = at::addmm(t[1], s, t[0].t());
    atomic = at::addmm(t[3], at::silu(hd.pre_o), t[2].t()).reshape({-1});
  }
  energy = at::empty({G}, fopt);
  XCALL(xeq_segment_sum(dt, atomic.data_ptr(), (const int64_t*)ptr64.data_ptr(), G, 1, energy.data_ptr(), st));
}

// EnergyReadout.backward / EnergyHead.backward: dE/ds from dE_i/d atomic_i = 1.  The fused form seeds the pass with MINUS one
// (minus_one above): everything behind it is then minus the gradient, and forces and virial come out without a negation
Tensor energy_readout_bwd(const Hyper& hy, const Tensor* t, const HeadSaved& hd) {
  Tensor g_s;
  if (hd.fused) {
    // (seed) x d atomic_i / d s_i, the row saved by the forward launch
    const int64_t N = hd.jac.size(0);
    const Tensor seed = minus_one(hd.jac.options());
    g_s = at::empty_like(hd.jac);
    XCALL(xeq_head_bwd(hd.jac.data_ptr(), N, hy.F, nullptr, 0, seed.data_ptr(), 0, nullptr, g_s.data_ptr(), cur_stream()));
  } else if (hd.native) {
    const int64_t N = hd.pre_o.size(0);
    Tensor g_hidden = at::empty_like(hd.pre_o);
    XCALL(xeq_head_bwd_hidden(hd.pre_o.data_ptr(), N, (int)hd.pre_o.size(1), t[2].data_ptr(), nullptr, g_hidden.data_ptr(), cur_stream()));
    g_s = linear_bwd(g_hidden, t[0], t[1]);
  } else {
    g_s = at::mm(at::silu_backward(t[2].expand({hd.pre_o.size(0), t[2].size(1)}), hd.pre_o), t[0]);
  }
  return g_s;
}

// ops.EdgeVectors.backward: dL/dvec -> dL/dpos (forces) and sym(sum_e vec_e (x) dE/dvec_e) per graph (virial).  negated: g_vec is
// minus the gradient already; undefined: zero
void edge_vectors_bwd_and_virial(Graph& g, const Tensor& vec, Tensor g_vec, const Tensor& ptr64, bool compute_forces,
                                 bool compute_virial, bool negated, Tensor& forces, Tensor& virial) {
  if (!g_vec.defined()) g_vec = at::zeros_like(vec);
  g_vec = g_vec.contiguous();
  const int64_t G = ptr64.numel() - 1;
  const auto fopt = vec.options();
  const int dt = dcode(vec);
  void* st = cur_stream();
  if (compute_forces) {
    Tensor grad_pos = at::empty({g.N, 3}, fopt);
    XCALL(xeq_edge_vectors_bwd(dt, g_vec.data_ptr(), g.N, (const int32_t*)g.c_rowptr.data_ptr(),
                               g.c_perm.defined() ? (const int32_t*)g.c_perm.data_ptr() : nullptr,
                               (const int32_t*)g.rev_rowptr().data_ptr(), (const int32_t*)g.rev_perm().data_ptr(), grad_pos.data_ptr(), st));
    forces = negated ? grad_pos : grad_pos.neg();
  }
  if (compute_virial) {   // edges walked center-sorted
    Tensor outer = (vec.unsqueeze(2) * g_vec.unsqueeze(1)).reshape({-1, 9});
    if (g.c_perm.defined()) outer = outer.index_select(0, g.c_perm.to(at::kLong));
    const Tensor eptr = g.c_rowptr.to(at::kLong).index_select(0, ptr64).contiguous();
    outer = outer.contiguous();
    Tensor msum = at::empty({G, 9}, fopt);
    XCALL(xeq_segment_sum(dt, outer.data_ptr(), (const int64_t*)eptr.data_ptr(), G, 9, msum.data_ptr(), st));
    msum = msum.view({G, 3, 3});
    virial = 0.5 * (msum + msum.transpose(1, 2));
    if (!negated) virial = virial.neg();
  }
}

// ---------------------------------------------------------------------------------------------- the evaluation
std::vector<Tensor> xpainn_eval_impl(const Tensor& pos_in, const Tensor& atomic_numbers, const Tensor& edge_index, const Tensor& ptr,
                                     const c10::optional<Tensor>& cell_o, const c10::optional<Tensor>& cell_offsets_o,
                                     const std::vector<Tensor>& prm, const std::vector<int64_t>& ip, const std::vector<double>& fp,
                                     bool center_sorted, bool symmetric, bool compute_forces, bool compute_virial,
                                     const c10::optional<Tensor>& charge_o, const c10::optional<Tensor>& spin_o) {
  need_hip(pos_in, "pos");
  need_hip(edge_index, "edge_index");
  TORCH_CHECK(ip.size() >= 10 && fp.size() >= 2, "xeq::xpainn_eval: malformed hyper-parameter lists");
  const Hyper hy{(int)ip[0], {(int)ip[1], (int)ip[2], (int)ip[3]}, (int)ip[4], (int)ip[5], (int)ip[6], (int)ip[7], (int)ip[8], (int)ip[9], fp[0], fp[1]};
  // charge / spin embeddings (nn/electronic.py): flags at the end of iparams, parameters behind the head tail
  const bool el_charge = ip.size() >= 12 && ip[10] != 0, el_spin = ip.size() >= 12 && ip[11] != 0;
  const int64_t n_prm = P_BLOCK0 + (int64_t)P_PER_BLOCK * hy.blocks + 4 + P_ELECTRONIC * ((int)el_charge + (int)el_spin);
  TORCH_CHECK((int64_t)prm.size() == n_prm, "xeq::xpainn_eval: expected ", n_prm, " parameter tensors, got ", prm.size());
  TORCH_CHECK(edge_index.dim() == 2 && edge_index.size(0) == 2 && edge_index.scalar_type() == at::kLong, "edge_index must be int64 [2, E]");
  const Tensor pos = pos_in.detach().contiguous();
  const auto fopt = pos.options();
  const int dt = dcode(pos);
  const int64_t N = pos.size(0), G = ptr.numel() - 1;
  const int F = hy.F;
  const Tensor ptr64 = ptr.to(at::kLong).contiguous();
  void* st = cur_stream();
  // a module runs when the model has it AND the per-graph value is given (the module is the identity otherwise, electronic.py:31-32)
  const bool run_charge = el_charge && charge_o.has_value() && charge_o->defined();
  const bool run_spin = el_spin && spin_o.has_value() && spin_o->defined();
  const bool run_el = run_charge || run_spin;
  if (run_el) {
    need_hip(run_charge ? *charge_o : *spin_o, run_charge ? "charge" : "spin");
    TORCH_CHECK(dt == XEQ_F32 && xeq_electronic_supported(XEQ_F32, F), "xeq::xpainn_eval: the charge / spin embeddings run in f32 with "
                "node_dim a multiple of 32, <= 256: use the Python modules");
  }

  const Tensor ei_c = edge_index.contiguous();
  const int64_t E = ei_c.size(1);

  // ---- sorted views of the edge list (ops.EdgeGraph), then the edge geometry (nn/basic.py:110-131): the order of the Python front
  // (nn/basic.py::compute_edge_data builds the graph first), so that both fronts issue ONE launch sequence
  // (tests/test_gpu_interface.py::test_both_fronts_issue_the_same_launch_sequence)
  Tensor cell, cell_offsets, batch;
  const bool has_cell = cell_o.has_value() && cell_o->defined();
  if (has_cell) {
    TORCH_CHECK(cell_offsets_o.has_value() && cell_offsets_o->defined(), "cell without cell_offsets");
    cell = cell_o->to(pos.scalar_type()).contiguous();
    cell_offsets = cell_offsets_o->to(pos.scalar_type()).contiguous();
  }
  Graph g = build_graph(ei_c, N, center_sorted, symmetric, has_cell ? &cell_offsets : nullptr);
  if (has_cell) {
    if (G > 1) {
      const Tensor counts = ptr64.slice(0, 1) - ptr64.slice(0, 0, G);
      batch = at::repeat_interleave(at::arange(G, ptr64.options()), counts, 0, N);
    }
  }
  Tensor vec = at::empty({E, 3}, fopt), dist = at::empty({E}, fopt);
  XCALL(xeq_edge_vectors_fwd(dt, pos.data_ptr(), (const int64_t*)ei_c.data_ptr(), E, has_cell ? cell.data_ptr() : nullptr,
                             has_cell ? cell_offsets.data_ptr() : nullptr, batch.defined() ? (const int64_t*)batch.data_ptr() : nullptr,
                             vec.data_ptr(), dist.data_ptr(), st));

  // ---- which message kernels (ops.select_message_impl, without the generic form).  The family rule is the C ABI's
  // (xeq_message_auto_family: the Python modules ask the same function); this operator carries the wq and sb sequences
  const int family = xeq_message_auto_family(dt, N, E, hy.B, F, hy.mul);
  TORCH_CHECK(family == XEQ_FAMILY_WQ || family == XEQ_FAMILY_SB,
              "xeq::xpainn_eval: this configuration / size needs the generic message kernels: use the Python modules");
  const bool wq = family == XEQ_FAMILY_WQ;
  const bool want_bwd = compute_forces || compute_virial;
  auto Q = [&](int b) { return &prm[P_BLOCK0 + P_PER_BLOCK * b]; };   // block b's parameters; b = blocks: the head's

  // ---- embedding, charge / spin embeddings, the first block's front half where the embedding's gather has not made it, edge records:
  // the order of the Python front (the record launch sits in ops.message_forward, behind MessageBlock's norms and scalar_mlp)
  std::vector<MsgSaved> msv(hy.blocks + 1);   // (+ 1: embed_and_first_front takes a reference also when the model has no block)
  std::vector<UpdSaved> usv(hy.blocks);
  Tensor x = at::zeros({N, hy.D()}, fopt);
  Tensor s = embed_and_first_front(hy, prm, atomic_numbers, x, wq, run_el, msv[0]);
  if (run_el) {
    const bool has[2] = {el_charge, el_spin};
    const Tensor* const total[2] = {run_charge ? &*charge_o : nullptr, run_spin ? &*spin_o : nullptr};
    s = electronic_fwd(hy, &prm[P_BLOCK0 + P_PER_BLOCK * hy.blocks + 4], has, total, s, ptr64);
  }
  if (hy.blocks > 0 && !msv[0].h.defined()) message_front_fwd(hy, Q(0), s, x, msv[0]);
  if (msv[0].tab_z.defined()) {   // the first block's table form: every record launch of the evaluation writes the plans' table rows
    g.table_z = msv[0].tab_z;
    g.table_rows = msv[0].tab_h.size(0);
  }
  // (wq, mirror walk: the reverse pass runs over the same plan, its derivative records come out of the same launch)
  edge_basis(hy, g, vec, prm[3], prm[4], wq, false, g.mirror && want_bwd);

  // ---- the blocks.  Fused node blocks: f32, the default layout, layer norms on (nn/nodeblock.py::supported)
  const bool nb_ok = dt == XEQ_F32 && hy.layer_norm && xeq_node_block_supported(XEQ_F32, F, hy.mul) && xeq_node_block_auto(N);
  for (int b = 0; b < hy.blocks; ++b) {
    const bool last = b == hy.blocks - 1;
    message_block_fwd(hy, g, Q(b), wq, b == 0, msv[b], s, x);
    if (nb_ok) node_block_fwd(hy, Q(b), last ? nullptr : Q(b + 1), usv[b], last ? nullptr : &msv[b + 1], s, x);
    else update_block_fwd(hy, Q(b), last, usv[b], s, x);
  }
  HeadSaved head;
  Tensor atomic, energy;
  energy_readout_fwd(hy, Q(hy.blocks), s, ptr64, want_bwd, head, atomic, energy);

  Tensor forces, virial;
  if (want_bwd) {
    // ---- explicit reverse pass: dE/ds of the head, then the blocks backwards, then the edge geometry (nn/basic.py:143-199)
    Tensor g_s = energy_readout_bwd(hy, Q(hy.blocks), head);
    Tensor g_x;   // undefined = zero: the head reads the scalars only, the last block's equivariant output has no consumer
    EdgeGrad eg;
    eg.defer = wq && hy.blocks <= XEQ_WQ_MAX_PART_SETS;
    if (wq && !g.mirror) edge_basis(hy, g, vec, prm[3], prm[4], true, true, true);
    Tensor pend_gh, pend_gxhat;   // gradients of the next block's (h, xhat): reversed by the node block of the update in front of it
    for (int b = hy.blocks - 1; b >= 0; --b) {
      const bool last = b == hy.blocks - 1;
      if (nb_ok) {
        node_block_bwd(hy, Q(b), last ? nullptr : Q(b + 1), usv[b], last ? nullptr : &msv[b + 1], pend_gh, pend_gxhat, g_s, g_x);
        pend_gh = Tensor();
        pend_gxhat = Tensor();
      } else {
        update_block_bwd(hy, Q(b), usv[b], g_s, g_x);
      }
      Tensor g_h, g_xhat;
      message_block_bwd(hy, g, Q(b), wq, b == 0, vec, msv[b], g_s, g_x, g_h, g_xhat, eg);
      if (b == 0) break;   // the first block's node features (embedding, zeros) do not depend on the positions
      if (nb_ok) {         // the front half of this block is reversed by the node block of update b - 1; g_s, g_x: the residual path
        pend_gh = g_h;
        pend_gxhat = g_xhat;
      } else {
        message_front_bwd(hy, Q(b), msv[b], g_h, g_xhat, g_s, g_x);
      }
    }
    edge_vectors_bwd_and_virial(g, vec, eg.total, ptr64, compute_forces, compute_virial, head.fused, forces, virial);
  }
  if (!forces.defined()) forces = at::empty({0, 3}, fopt);
  if (!virial.defined()) virial = at::empty({0, 3, 3}, fopt);
  return {energy, atomic, forces, virial};
}

// autograd wrapper: energy (and nothing else) is differentiable w.r.t. pos; backward = -forces * grad_energy[graph]
class XpainnEvalFn : public torch::autograd::Function<XpainnEvalFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& pos, const Tensor& atomic_numbers, const Tensor& edge_index,
                               const Tensor& ptr, const c10::optional<Tensor>& cell, const c10::optional<Tensor>& cell_offsets,
                               std::vector<Tensor> prm, std::vector<int64_t> ip, std::vector<double> fp, bool center_sorted,
                               bool symmetric, bool compute_forces, bool compute_virial, const c10::optional<Tensor>& charge,
                               const c10::optional<Tensor>& spin) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const bool need = compute_forces || pos.requires_grad();
    auto out = xpainn_eval_impl(pos, atomic_numbers, edge_index, ptr, cell, cell_offsets, prm, ip, fp, center_sorted, symmetric, need,
                                compute_virial, charge, spin);
    ctx->save_for_backward({out[2], ptr});
    ctx->mark_non_differentiable({out[1], out[2], out[3]});
    return {out[0], out[1], out[2], out[3]};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor& forces = saved[0];
    const Tensor ptr = saved[1].to(at::kLong);
    Tensor g_pos;
    if (grads[0].defined() && forces.size(0) > 0) {
      const int64_t G = ptr.numel() - 1, N = forces.size(0);
      const Tensor counts = ptr.slice(0, 1) - ptr.slice(0, 0, G);
      const Tensor per_atom = at::repeat_interleave(grads[0].reshape({-1}), counts, 0, N);
      g_pos = forces.neg() * per_atom.unsqueeze(1);
    }
    variable_list r(15);
    r[0] = g_pos;
    return r;
  }
};

std::vector<Tensor> xpainn_eval(const Tensor& pos, const Tensor& atomic_numbers, const Tensor& edge_index, const Tensor& ptr,
                                const c10::optional<Tensor>& cell, const c10::optional<Tensor>& cell_offsets, std::vector<Tensor> prm,
                                std::vector<int64_t> ip, std::vector<double> fp, bool center_sorted, bool symmetric,
                                bool compute_forces, bool compute_virial, const c10::optional<Tensor>& charge,
                                const c10::optional<Tensor>& spin) {
  return XpainnEvalFn::apply(pos, atomic_numbers, edge_index, ptr, cell, cell_offsets, prm, ip, fp, center_sorted, symmetric,
                             compute_forces, compute_virial, charge, spin);
}

// count -> scan -> size -> fill on a filled search record (include/xeq.h: xeq_neighbor_search), the host path of both registered
// list operators: one device-to-host read of the edge count, as the reference's nonzero().  -> (edge_index [2, E], cell_offsets
// [E, 3] for the periodic kinds, else undefined, rowptr [N + 1])
static std::tuple<Tensor, Tensor, Tensor> neighbor_list(const xeq_neighbor_search& s, const Tensor& pos, const Tensor& ptr64, const char* who) {
  const int64_t N = s.n_nodes;
  Tensor deg = i32(N, ptr64), rowptr = i32(N + 1, ptr64);
  void* st = cur_stream();
  XCALL(xeq_neighbors_count(&s, (int32_t*)deg.data_ptr(), st));
  const int64_t scan_bytes = xeq_exclusive_scan_i32_workspace(N);
  TORCH_CHECK(scan_bytes >= 0, who, ": too many nodes");
  Tensor scan_work = at::empty({std::max<int64_t>(scan_bytes, 1)}, pos.options().dtype(at::kByte));
  XCALL(xeq_exclusive_scan_i32_ws((const int32_t*)deg.data_ptr(), N, (int32_t*)rowptr.data_ptr(), scan_work.data_ptr(), scan_bytes, st));
  const int64_t E = N > 0 ? (int64_t)rowptr[N].item<int32_t>() : 0;
  Tensor ei = at::empty({2, E}, ptr64.options()), cell_offsets;
  if (s.kind >= XEQ_NEIGHBORS_PBC_ALL) cell_offsets = at::empty({E, 3}, pos.options());
  XCALL(xeq_neighbors_fill(&s, (const int32_t*)rowptr.data_ptr(), E, nullptr, (int64_t*)ei.data_ptr(),
                           cell_offsets.defined() ? cell_offsets.data_ptr() : nullptr, st));
  return {ei, cell_offsets, rowptr};
}

// open-boundary neighbour list (the pair sweep)
std::tuple<Tensor, Tensor> radius_graph(const Tensor& pos_in, const Tensor& ptr, double cutoff) {
  need_hip(pos_in, "pos");
  const Tensor pos = pos_in.detach().contiguous();
  const Tensor ptr64 = ptr.to(at::kLong).contiguous();
  xeq_neighbor_search s = {};
  s.dtype = dcode(pos), s.kind = XEQ_NEIGHBORS_OPEN_SWEEP, s.n_graphs = ptr64.numel() - 1, s.n_nodes = pos.size(0), s.cutoff = cutoff;
  s.pos = pos.data_ptr(), s.ptr = (const int64_t*)ptr64.data_ptr();
  const auto out = neighbor_list(s, pos, ptr64, "xeq::radius_graph");
  return {std::get<0>(out), std::get<2>(out)};
}

// periodic neighbour list of ONE system (data/radius_graph.py:195-275): positions are not wrapped, cell [3, 3], pbc [3].
// The twin of data.radius_graph.single_radius_graph of this package: the same host tables (xeq_pbc_image_counts /
// xeq_pbc_tables_host) and the same image-pruned search kernels, hence the same list bit for bit.  Two round trips, as there:
// the cell (9 numbers) comes to the host for the image counts, and the edge count sizes the output (the reference's nonzero()).
std::tuple<Tensor, Tensor, Tensor> radius_graph_pbc(const Tensor& pos_in, const Tensor& cell_in, const Tensor& pbc_in, double cutoff) {
  need_hip(pos_in, "pos");
  TORCH_CHECK(cell_in.dim() == 2 && cell_in.size(0) == 3 && cell_in.size(1) == 3, "xeq::radius_graph_pbc: cell must be [3, 3]");
  TORCH_CHECK(pbc_in.numel() == 3, "xeq::radius_graph_pbc: pbc must hold three flags");
  const Tensor pos = pos_in.detach().contiguous();
  const int dt = dcode(pos);
  const int64_t N = pos.size(0);
  const Tensor cell_h = cell_in.detach().to(pos.scalar_type()).to(at::kCPU).contiguous();   // round trip 1
  const Tensor pbc_h = pbc_in.detach().to(at::kCPU).to(at::kInt).reshape({3}).contiguous();
  const int32_t pbc[3] = {pbc_h.data_ptr<int32_t>()[0] != 0, pbc_h.data_ptr<int32_t>()[1] != 0, pbc_h.data_ptr<int32_t>()[2] != 0};
  int32_t reps[3];
  XCALL(xeq_pbc_image_counts(dt, cell_h.data_ptr(), 1, pbc, cutoff, reps));
  const int64_t nc = (int64_t)(2 * reps[0] + 1) * (2 * reps[1] + 1) * (2 * reps[2] + 1), n_tab = 6 * nc + 12;
  Tensor tab_h = at::empty({n_tab}, cell_h.options());
  XCALL(xeq_pbc_tables_host(dt, cell_h.data_ptr(), 1, reps, cutoff, tab_h.data_ptr(), n_tab));
  const Tensor tab = tab_h.to(pos.device());                                                 // one upload
  const Tensor grid = tab.narrow(0, 0, 3 * nc), offs = tab.narrow(0, 3 * nc, 3 * nc), recip = tab.narrow(0, 6 * nc, 9),
               thr = tab.narrow(0, 6 * nc + 9, 3);
  const Tensor ptr64 = at::tensor({(int64_t)0, N}, at::TensorOptions().dtype(at::kLong)).to(pos.device());
  const Tensor shift = at::zeros_like(pos);
  xeq_neighbor_search s = {};
  s.dtype = dt, s.kind = XEQ_NEIGHBORS_PBC_PRUNED, s.n_graphs = 1, s.n_nodes = N, s.n_cells = nc, s.cutoff = cutoff;
  s.reps[0] = reps[0], s.reps[1] = reps[1], s.reps[2] = reps[2];
  s.pos = pos.data_ptr(), s.ptr = (const int64_t*)ptr64.data_ptr(), s.img = offs.data_ptr(), s.cells = grid.data_ptr();
  s.shift = shift.data_ptr(), s.recip = recip.data_ptr(), s.thr = thr.data_ptr();
  return neighbor_list(s, pos, ptr64, "xeq::radius_graph_pbc");                              // round trip 2: the edge count
}

// ---------------------------------------------------------------------------------------------- linear layers of the training pass
// y = x W^T (+ b) as an autograd node whose reverse pass is written with itself and with XeqWGradFn (dL/dx = g W, dL/dW = g^T x), so
// every order of derivative stays on these two products, and every reduction over the N rows -- which the library's GEMMs run at a
// tenth of their rate for [576 x N] x [N x 128] and the like -- goes to xeq_wgrad (fp32).  Python twin: nn/training_ops.py LinearFn /
// WGradFn (same arithmetic; a C++ node costs the host a fifth of a Python one, which is what decides a host-launched training step).
struct XeqWGradFn;
Tensor xeq_wgrad_apply(const Tensor& a, const Tensor& b);

struct XeqLinearFn : public torch::autograd::Function<XeqLinearFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& W, const std::optional<Tensor>& b) {
    ctx->save_for_backward({x, W});
    const bool has_bias = b.has_value() && b->defined();
    ctx->saved_data["has_bias"] = has_bias;
    return has_bias ? at::addmm(*b, x, W.t()) : at::mm(x, W.t());
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &x = saved[0], &W = saved[1], &go = g[0];
    Tensor dx, dW, db;
    if (ctx->needs_input_grad(0)) dx = XeqLinearFn::apply(go, W.t(), std::optional<Tensor>());
    if (ctx->needs_input_grad(1)) dW = xeq_wgrad_apply(go, x);
    if (ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(2)) db = go.sum(0);
    return {dx, dW, db};
  }
};

struct XeqWGradFn : public torch::autograd::Function<XeqWGradFn> {   // a^T b over the rows: a [N, M], b [N, K] -> [M, K]
  static Tensor forward(AutogradContext* ctx, const Tensor& a, const Tensor& b) {
    ctx->save_for_backward({a, b});
    if (!(a.is_cuda() && a.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat && a.dim() == 2 && b.dim() == 2 && a.size(0) == b.size(0)))
      return at::mm(a.t(), b);
    const Tensor ac = a.stride(1) == 1 ? a : a.contiguous(), bc = b.stride(1) == 1 ? b : b.contiguous();
    const int64_t n = ac.size(0);
    const int M = (int)ac.size(1), K = (int)bc.size(1);
    const int chunks = xeq_wgrad_chunks(n, M, K);
    Tensor parts = at::empty({chunks, (int64_t)M * K}, ac.options());
    XCALL(xeq_wgrad(ac.data_ptr(), ac.stride(0), bc.data_ptr(), bc.stride(0), n, M, K, 0, chunks, parts.data_ptr(), cur_stream()));
    return (chunks > 1 ? parts.sum(0) : parts[0]).view({M, K});
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &a = saved[0], &b = saved[1], &U = g[0];
    Tensor da, db;
    if (ctx->needs_input_grad(0)) da = XeqLinearFn::apply(b, U, std::optional<Tensor>());       // b U^T
    if (ctx->needs_input_grad(1)) db = XeqLinearFn::apply(a, U.t(), std::optional<Tensor>());   // a U
    return {da, db};
  }
};
Tensor xeq_wgrad_apply(const Tensor& a, const Tensor& b) { return XeqWGradFn::apply(a, b); }

Tensor linear_op(const Tensor& x, const Tensor& W, const std::optional<Tensor>& b) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2 && x.size(1) == W.size(1), "xeq::linear: x [N, K], W [M, K]");
  return XeqLinearFn::apply(x, W, b);
}

}  // namespace

TORCH_LIBRARY(xeq, m) {
  m.def(
      "xpainn_eval(Tensor pos, Tensor atomic_numbers, Tensor edge_index, Tensor ptr, Tensor? cell, Tensor? cell_offsets, "
      "Tensor[] params, int[] iparams, float[] fparams, bool center_sorted, bool symmetric, bool compute_forces, "
      "bool compute_virial, Tensor? charge=None, Tensor? spin=None) -> Tensor[]");
  m.def("radius_graph(Tensor pos, Tensor ptr, float cutoff) -> (Tensor, Tensor)");
  m.def("radius_graph_pbc(Tensor pos, Tensor cell, Tensor pbc, float cutoff) -> (Tensor, Tensor, Tensor)");
  m.def("linear(Tensor x, Tensor W, Tensor? b) -> Tensor", linear_op);   // differentiable to every order (XeqLinearFn / XeqWGradFn)
}

TORCH_LIBRARY_IMPL(xeq, Autograd, m) { m.impl("xpainn_eval", xpainn_eval); }
TORCH_LIBRARY_IMPL(xeq, CompositeExplicitAutograd, m) {
  m.impl("radius_graph", radius_graph);
  m.impl("radius_graph_pbc", radius_graph_pbc);
}
