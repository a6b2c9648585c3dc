from .ase_calculator import XequiCalculator
from .md_model import PaiNNGMX, PaiNNLMP, XPaiNNGMX, XPaiNNLMP, resolve_jit_model

__all__ = ["XPaiNNLMP", "XPaiNNGMX", "PaiNNLMP", "PaiNNGMX", "resolve_jit_model", "XequiCalculator"]
