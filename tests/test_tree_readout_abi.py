"""CPU: the tree read-out entry points (ao_tree_lookup / ao_tree_pv / ao_tree_stats) are exported by the built library and
bound by alpha_omok_amd._lib; the ABI version did not move (the calls are additive)."""
import ctypes

READOUT = ("ao_tree_lookup", "ao_tree_pv", "ao_tree_stats")


def test_library_exports_tree_readout():
    from alpha_omok_amd import build
    raw = ctypes.CDLL(build.build())
    for name in READOUT:
        assert hasattr(raw, name), "libomok_hip.so does not export %s" % name


def test_lib_binds_tree_readout():
    from alpha_omok_amd import _lib
    lib = _lib.load(build_if_missing=False)
    for name in READOUT:
        assert name in _lib.SYMBOLS
        res, args = _lib.SYMBOLS[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert len(_lib.SYMBOLS["ao_tree_lookup"][1]) == 14
    assert len(_lib.SYMBOLS["ao_tree_pv"][1]) == 7
    assert len(_lib.SYMBOLS["ao_tree_stats"][1]) == 3
    assert (_lib.AO_NODE_ABSENT, _lib.AO_NODE_LEAF, _lib.AO_NODE_TERMINAL, _lib.AO_NODE_EXPANDED) == (0, 1, 2, 3)
    assert lib.ao_abi_version() == 2


def test_python_layers_expose_tree_readout():
    from alpha_omok_amd import agents, engine
    for name in ("tree_lookup", "principal_variations", "tree_stats"):
        assert callable(getattr(engine.Engine, name))
    for name in ("principal_variation", "tree_depth"):
        assert callable(getattr(agents.ZeroAgent, name))
    for name in ("__getitem__", "__contains__", "__len__", "clear"):
        assert hasattr(agents._TreeView, name)
    # without an engine (no search yet) the view is the reference's empty dict
    ag = agents.ZeroAgent.__new__(agents.ZeroAgent)
    ag._engine = None
    view = agents._TreeView(ag)
    assert (0,) not in view and len(view) == 0
    try:
        view[(0,)]
    except KeyError:
        pass
    else:
        raise AssertionError("an empty tree must raise KeyError")
    assert ag.tree_depth() == 0 and len(ag.principal_variation()[0]) == 0
