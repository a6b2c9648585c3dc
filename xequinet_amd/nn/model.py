"""Model assembly -- mirror of ``xequinet/nn/model.py`` for the XPaiNN energy path:
``BaseModel.forward(data, compute_forces, compute_virial)`` (nn/model.py:26-46),
``XPaiNN`` (:49-122), ``XPaiNNEwald`` (:125-176), ``PaiNN`` (:261-307), ``resolve_model`` (:310-318), ``load_model`` (:321-351)."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Union

import torch
import torch.nn as nn

from . import training
from .. import keys as keys_
from .basic import compute_edge_data, compute_properties
from .electronic import ChargeEmbedding, SpinEmbedding
from .output import EnergyOut, resolve_output
from .xpainn import XEmbedding, XPainnMessage, XPainnUpdate

# e3nn bookkeeping entries of reference checkpoints that have no counterpart here
# (weight-less TensorProducts register an empty `weight` and an `output_mask` buffer)
_E3NN_ONLY = (".rsh_conv.", ".tp.", ".scalar_mul.", ".sph_harm.", ".output_mask", "._", ".invariant.tp", ".equidot.tp")


class BaseModel(nn.Module):
    cutoff_radius: float

    def __init__(self) -> None:
        super().__init__()
        self.mods = nn.ModuleDict()
        self.extra_properties = []
        self.native_training = True   # False: an energy-only training pass takes the differentiable form too (nn/training.py)

    def forward(
        self,
        data: Dict[str, torch.Tensor],
        compute_forces: bool = True,
        compute_virial: bool = False,
    ) -> Dict[str, torch.Tensor]:
        # a training pass (train mode, parameters asking for gradients) whose result carries forces or a virial runs every block
        # in its differentiable form so that the force evaluation can itself be differentiated (create_graph=training,
        # nn/basic.py:143-159); with energies only (no second order) the blocks stay on the fused kernels and return their
        # parameter gradients themselves (nn/fused.py); everything else is the fused inference path
        if (compute_forces or compute_virial) and not any(isinstance(m, EnergyOut) for m in self.mods.values()):
            raise KeyError(f"forces / virial are derivatives of {keys_.TOTAL_ENERGY!r}: this model has no \"energy\" output head "
                           f"(heads: {[k for k in self.mods if k.startswith('output_')]}); call it with compute_forces=False")
        train_pass = training.wants_training_pass(self)
        native = train_pass and not compute_forces and not compute_virial and self.native_training and training.native_pass_supported(self)
        data[training.PARAM_GRADS] = native
        train_pass = train_pass and not native
        data[training.TRAIN_PASS] = train_pass
        if train_pass:
            data = training.edge_data(data, compute_forces=compute_forces, compute_virial=compute_virial)
        else:
            data = compute_edge_data(data=data, compute_forces=compute_forces, compute_virial=compute_virial)
            # one edge-gradient launch for all message blocks of this evaluation (ops.EdgeGradDeferral): a fresh collector per call
            from .. import keys, ops

            g = data.get(keys.EDGE_GRAPH)
            if g is not None:
                g.edge_grad_deferral = ops.EdgeGradDeferral() if (compute_forces or compute_virial) and not native else None
        for mod in self.mods.values():
            data = mod(data)
        result = compute_properties(
            data=data,
            compute_forces=compute_forces,
            compute_virial=compute_virial,
            training=train_pass,
            extra_properties=self.extra_properties,
        )
        return result

    def load_reference_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """Load a reference checkpoint's ``ckpt['model']``: e3nn-only bookkeeping
        entries are dropped, everything else must match strictly."""
        own = self.state_dict()
        kept = {}
        for k, v in state_dict.items():
            if k in own:
                kept[k] = v.reshape(own[k].shape) if v.numel() == own[k].numel() else v
            elif not any(tag in k for tag in _E3NN_ONLY):
                raise KeyError(f"unexpected key in reference state dict: {k}")
        missing = [k for k in own if k not in kept]
        if missing:
            raise KeyError(f"missing keys in reference state dict: {missing}")
        self.load_state_dict(kept, strict=True)


class XPaiNN(BaseModel):
    """eXtended PaiNN (nn/model.py:49-122), with the optional charge / spin embeddings (nn/electronic.py)."""

    def __init__(self, **kwargs) -> None:
        super().__init__()
        node_dim: int = kwargs.get("node_dim", 128)
        node_irreps: str = kwargs.get("node_irreps", "128x0e + 64x1o + 32x2e")
        embed_basis: str = kwargs.get("embed_basis", "gfn2-xtb")
        aux_basis: str = kwargs.get("aux_basis", "aux56")
        num_basis: int = kwargs.get("num_basis", 20)
        rbf_kernel: str = kwargs.get("rbf_kernel", "bessel")
        cutoff: float = kwargs.get("cutoff", 5.0)
        cutoff_fn: str = kwargs.get("cutoff_fn", "cosine")
        action_blocks: int = kwargs.get("action_blocks", 3)
        activation: str = kwargs.get("activation", "silu")
        layer_norm: bool = kwargs.get("layer_norm", True)
        charge_embed: bool = kwargs.get("charge_embed", False)
        spin_embed: bool = kwargs.get("spin_embed", False)
        output_modes: Union[str, List[str]] = kwargs.get("output_modes", ["energy"])

        self.cutoff_radius = cutoff
        self.mods["embedding"] = XEmbedding(
            node_dim=node_dim, node_irreps=node_irreps, embed_basis=embed_basis, aux_basis=aux_basis,
            num_basis=num_basis, rbf_kernel=rbf_kernel, cutoff=cutoff, cutoff_fn=cutoff_fn,
        )
        if charge_embed:   # nn/model.py:85-96: charge before spin, both between the embedding and the first message block
            self.mods["charge_embedding"] = ChargeEmbedding(node_dim=node_dim, activation=activation)
        if spin_embed:
            self.mods["spin_embedding"] = SpinEmbedding(node_dim=node_dim, activation=activation)
        for i in range(action_blocks):
            self.mods[f"message_{i}"] = XPainnMessage(
                node_dim=node_dim, node_irreps=node_irreps, num_basis=num_basis, activation=activation, layer_norm=layer_norm,
            )
            self.mods[f"update_{i}"] = XPainnUpdate(
                node_dim=node_dim, node_irreps=node_irreps, activation=activation, layer_norm=layer_norm,
            )
        # the embedding gathers the first message block's front half with the node scalars -- not behind a charge / spin embedding:
        # there the first block's scalars no longer depend on the element alone (the block still sees the zero-equivariant tag)
        if action_blocks > 0 and not (charge_embed or spin_embed):
            self.mods["embedding"]._next_message = [self.mods["message_0"]]
        for i in range(action_blocks - 1):   # an update block launches the front half of the message block behind it (nn/fused.py::NodeBlock)
            self.mods[f"update_{i}"]._next_message = [self.mods[f"message_{i + 1}"]]
        if output_modes is None:
            output_modes = ["energy"]
        elif isinstance(output_modes, str) or not isinstance(output_modes, Iterable):
            output_modes = [output_modes]
        for mode in output_modes:
            output = resolve_output(mode, **kwargs)
            self.mods[f"output_{mode}"] = output
            self.extra_properties.extend(output.extra_properties)
        # the heads built here read the node scalars only (nn/output.py:114-128), so the last update block's equivariant output has
        # no consumer: it is not computed (data[NODE_EQUIVARIANT] is None behind that block) and its gradient is not formed
        if action_blocks > 0 and all(not getattr(self.mods[f"output_{m}"], "reads_equivariant", False) for m in output_modes):
            self.mods[f"update_{action_blocks - 1}"].equivariant_output_unused = True


class XPaiNNEwald(XPaiNN):
    """XPaiNN with Ewald message passing (nn/model.py:125-176): behind every XPaiNN module, the output heads included, come
    ``ewald_initial``, ``ewald_0`` ... and a second set of heads ``ewald_output_<mode>``; the second energy head adds to the atomic
    energies of the first.  The eager model evaluates it (nn/ewald.py: kernels in f32 inference, the tensor form otherwise); the
    fronts that evaluate the energy chain alone refuse it (nn/output.py::refuse_ewald)."""

    def __init__(self, **kwargs) -> None:
        super().__init__(**kwargs)
        from .ewald import EwaldBlock, EwaldInitialNonPBC, EwaldInitialPBC

        node_dim: int = kwargs.get("node_dim", 128)
        activation: str = kwargs.get("activation", "silu")
        layer_norm: bool = kwargs.get("layer_norm", True)
        use_pbc: bool = kwargs.get("use_pbc", True)
        projection_dim: int = kwargs.get("projection_dim", 8)
        ewald_blocks: int = kwargs.get("ewald_blocks", 1)
        ewald_output_modes: Union[str, List[str]] = kwargs.get("ewald_output_mode", ["energy"])

        if use_pbc:
            num_k_points: List[int] = kwargs.get("num_k_points", [3, 3, 3])
            ewald_initial = EwaldInitialPBC(num_k_points=num_k_points, projection_dim=projection_dim)
        else:
            ewald_initial = EwaldInitialNonPBC(
                k_cutoff=kwargs.get("k_cutoff", 0.4), delta_k=kwargs.get("delta_k", 0.2), num_k_basis=kwargs.get("num_k_basis", 20),
                k_offset=kwargs.get("k_offset", None), projection_dim=projection_dim,
            )
        self.mods["ewald_initial"] = ewald_initial
        for i in range(ewald_blocks):
            self.mods[f"ewald_{i}"] = EwaldBlock(node_dim=node_dim, projection_dim=projection_dim, activation=activation, layer_norm=layer_norm)
        # the kernel form is all blocks or none: the initial module writes either the kernel geometry or the tensor form's tensors
        ewald_initial.kernel_consumers = all(self.mods[f"ewald_{i}"].kernel_shape_ok() for i in range(ewald_blocks))
        from .ewald import KERNEL_MAX_K

        n_k = (ewald_initial.k_index_product_set if use_pbc else ewald_initial.k_grid).shape[0]
        if n_k > KERNEL_MAX_K:   # say so once, here: the tensor form materialises the reference's [n_atoms, K, node_dim] tensors
            import warnings

            ewald_initial.kernel_consumers = False
            warnings.warn(f"XPaiNNEwald: {n_k} k-points exceed the Ewald kernels' cap of {KERNEL_MAX_K}; every evaluation takes the tensor form, "
                          f"which forms several [n_atoms, {n_k}, {node_dim}] tensors per block", stacklevel=2)
        if ewald_output_modes is None:
            ewald_output_modes = ["energy"]
        elif isinstance(ewald_output_modes, str) or not isinstance(ewald_output_modes, Iterable):   # a plain string is one mode
            ewald_output_modes = [ewald_output_modes]
        for mode in ewald_output_modes:
            output = resolve_output(mode, **kwargs)
            self.mods[f"ewald_output_{mode}"] = output
            self.extra_properties.extend(output.extra_properties)
        action_blocks: int = kwargs.get("action_blocks", 3)
        if action_blocks > 0 and any(getattr(self.mods[f"ewald_output_{m}"], "reads_equivariant", False) for m in ewald_output_modes):
            self.mods[f"update_{action_blocks - 1}"].equivariant_output_unused = False


class PaiNN(BaseModel):
    """PaiNN (nn/model.py:261-307): Embedding, action_blocks x (PainnMessage, PainnUpdate), the output heads.

    An inference evaluation (eval mode or frozen parameters) in f32 on the GPU runs the kernels of csrc/xeq_painn.hip with their
    explicit reverse passes; f64, CPU tensors, widths / activations without a kernel and every training pass run the tensor form of
    nn/painn.py, which autograd differentiates twice."""

    def __init__(self, **kwargs) -> None:
        super().__init__()
        from .painn import Embedding, PainnMessage, PainnUpdate

        node_dim: int = kwargs.get("node_dim", 128)
        embed_basis: str = kwargs.get("embed_basis", "gfn2-xtb")
        aux_basis: str = kwargs.get("aux_basis", "aux56")
        num_basis: int = kwargs.get("num_basis", 20)
        rbf_kernel: str = kwargs.get("rbf_kernel", "bessel")
        cutoff: float = kwargs.get("cutoff", 5.0)
        cutoff_fn: str = kwargs.get("cutoff_fn", "cosine")
        action_blocks: int = kwargs.get("action_blocks", 3)
        activation: str = kwargs.get("activation", "silu")
        output_modes: Union[str, List[str]] = kwargs.get("output_modes", ["energy"])

        self.cutoff_radius = cutoff
        self.action_blocks = action_blocks
        self.mods["embedding"] = Embedding(node_dim=node_dim, embed_basis=embed_basis, aux_basis=aux_basis, num_basis=num_basis,
                                           rbf_kernel=rbf_kernel, cutoff=cutoff, cutoff_fn=cutoff_fn)
        for i in range(action_blocks):
            self.mods[f"message_{i}"] = PainnMessage(node_dim=node_dim, num_basis=num_basis, activation=activation)
            self.mods[f"update_{i}"] = PainnUpdate(node_dim=node_dim, activation=activation)
        if output_modes is None:
            output_modes = ["energy"]
        elif isinstance(output_modes, str) or not isinstance(output_modes, Iterable):
            output_modes = [output_modes]
        from .output import EnergyOut

        for mode in output_modes:
            output = resolve_output(mode, **kwargs)
            if not isinstance(output, EnergyOut):   # forward evaluates the energy head alone in the tensor form (f64, CPU, training)
                raise NotImplementedError(f"PaiNN: output mode {mode!r} is not supported, this model has the energy head only")
            self.mods[f"output_{mode}"] = output
            self.extra_properties.extend(output.extra_properties)
        # the heads read the node scalars only: the last update block's vector output has no consumer and is not formed
        if action_blocks > 0 and all(not getattr(self.mods[f"output_{m}"], "reads_equivariant", False) for m in output_modes):
            self.mods[f"update_{action_blocks - 1}"].equivariant_output_unused = True

    def tensor_form(self, data: Dict[str, torch.Tensor]) -> bool:
        from . import painn

        pos = data[keys_.POSITIONS]
        return bool(training.wants_training_pass(self) or not pos.is_cuda or pos.dtype != torch.float32 or not painn.native_supported(self))

    def run_blocks(self, data: Dict[str, torch.Tensor], compute_forces: bool, compute_virial: bool):
        """Edge geometry, the blocks and the heads: (data with the energies still attached to autograd, whether the reverse pass
        must itself be differentiable).  ``forward`` derives forces / virial from it; a front whose caller differentiates the energy
        (interface/md_model.py) stops here."""
        from . import painn
        from .output import EnergyOut

        tensor_form = self.tensor_form(data)
        create_graph = tensor_form and training.wants_training_pass(self)
        data[painn.TENSOR_FORM] = tensor_form
        data[training.PARAM_GRADS] = False
        data[training.TRAIN_PASS] = False   # (the heads' own switch: the tensor form evaluates them here)
        if tensor_form:
            data = painn.tensor_edge_data(data, compute_forces=compute_forces, compute_virial=compute_virial)
        else:
            training.active(self, data)   # (says once that an eval-mode evaluation fills no parameter gradients)
            data = compute_edge_data(data=data, compute_forces=compute_forces, compute_virial=compute_virial)
            # a new collector per evaluation: a reverse pass that was cut short leaves nothing behind for the next one
            collector = painn._EdgeGrad() if (compute_forces or compute_virial) else None
            if collector is not None:
                collector.registered = self.action_blocks
            data[painn.EDGE_GRAD] = collector
            data["_xeq_painn_x_is_zero"] = True   # consumed by the first message block: its vector input is the embedding's zeros
        for mod in self.mods.values():
            if tensor_form and isinstance(mod, EnergyOut):
                data = painn.tensor_energy_out(mod, data)
            else:
                data = mod(data)
        return data, create_graph

    def forward(self, data: Dict[str, torch.Tensor], compute_forces: bool = True, compute_virial: bool = False) -> Dict[str, torch.Tensor]:
        data, create_graph = self.run_blocks(data, compute_forces, compute_virial)
        return compute_properties(data=data, compute_forces=compute_forces, compute_virial=compute_virial, training=create_graph,
                                  extra_properties=self.extra_properties)


def resolve_model(model_name: str, **kwargs) -> BaseModel:
    models_factory = {"xpainn": XPaiNN, "xpainn-ewald": XPaiNNEwald, "painn": PaiNN}
    if model_name.lower() not in models_factory:
        raise NotImplementedError(f"Unsupported model {model_name}")
    return models_factory[model_name.lower()](**kwargs)


def load_model(ckpt_file: str, device: Optional[torch.device] = None):
    """nn/model.py:321-351: rebuild the model from ``ckpt['config']`` and wrap it
    with the neighbour transform."""
    from ..data import NeighborTransform

    class ModelWithTransform:
        def __init__(self, model, transform, device):
            self.model = model
            self.transform = transform
            self.device = device

        def __call__(self, data, **kwargs):
            data = data.to(self.device)
            data = self.transform(data)
            return self.model(data.to_dict(), **kwargs)

    if device is None:
        device = torch.device("cuda")
    ckpt = torch.load(ckpt_file, map_location=device)
    model_config = ckpt["config"]
    model = resolve_model(model_config["model_name"], **model_config["model_kwargs"]).to(device)
    model.load_reference_state_dict(ckpt["model"])
    model.eval()
    return ModelWithTransform(model, NeighborTransform(model.cutoff_radius), device)
