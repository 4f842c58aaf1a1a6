"""facl_amd -- MI355X-native hot path of tangent-T/FACL's contrastive training step.

Host side mirrors the reference's Python interface for this path (same function / class
names, argument meaning and error behaviour); all compute runs in hand-written HIP kernels
behind the C ABI of ``libfacl_hip.so`` (include/facl_hip.h).  There is no CPU or eager
fallback: importing an op without the built library raises.
"""
__version__ = "0.1.0"


def __getattr__(name):
    """lib_path / load_library of facl_amd._lib on first use: it imports torch, which train_flags must not pay for."""
    if name in ("lib_path", "load_library"):
        from . import _lib
        return getattr(_lib, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
