"""xequinet_amd -- MI355X-native XPaiNN energy+force hot path (drop-in for the
corresponding pieces of X1X1010/XequiNet).  HIP kernels live in csrc/ behind the
C ABI of include/xeq.h; this package is the host-side mirror of the reference's
``nn.Module`` / functional interface.  There is no CPU fallback."""
from . import keys  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # hessian / hessian_vector_products (hessian.py), imported on first use: the package itself imports without the built library
    if name in ("hessian", "hessian_vector_products"):
        import importlib

        mod = importlib.import_module(".hessian", __name__)     # (binds the callable module as ``hessian``)
        return mod if name == "hessian" else mod.hessian_vector_products
    if name == "md":     # device-resident molecular dynamics (md.py), imported on first use for the same reason
        import importlib

        return importlib.import_module(".md", __name__)
    if name == "optimize":     # device-resident batched FIRE and L-BFGS minimisers (optimize.py), likewise
        import importlib

        return importlib.import_module(".optimize", __name__)
    if name == "vibrations":     # batched harmonic analysis and thermochemistry behind hessian() (vibrations.py), likewise
        import importlib

        return importlib.import_module(".vibrations", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
