"""alpha_omok_amd -- MI355X-native AlphaZero self-play engine for Omok.

Drop-in for the hot path of reinforcement-learning-kr/alpha_omok (ZeroAgent.get_pi /
main.self_play): batched MCTS over structure-of-arrays trees in HBM, hand-written HIP kernels
for gfx950, behind a C ABI (include/omok_hip.h).
"""
__version__ = "0.1.0"

__all__ = ["PositionBatch", "positions"]


def __getattr__(name):
    # resolved on first use: importing the package itself loads nothing (the library path is chosen when _lib is imported)
    if name == "PositionBatch":
        from .positions import PositionBatch
        return PositionBatch
    if name == "positions":
        import importlib
        return importlib.import_module(".positions", __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
