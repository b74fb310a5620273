"""The workspace-size cases of the enhance entry points: what tests/test_cabi.py (no device) and tests/test_gpu_enhance_plan.py
(sizes under a context's tuning) compute and hold against tests/golden/workspace_bytes.json.  The tables there were
recorded before plan_enhance became the one place that lays the workspace out; every later layout has to give the same bytes."""
import ctypes
import json
import os

from underwater_image_enhancement_amd import _lib

SIX, DICT = _lib.SURFACE_SIX, _lib.SURFACE_DICT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

# (5, 96, 136): a batch that 2, 3 and 4 all divide with a remainder, so every sub-batch split is ragged.
# (16, 1080, 1920): frames whose level-0 quadrant histograms come out of cast detection; (3, 131, 203): W % 8 != 0, they do not.
SHAPES = ((1, 1, 1), (2, 48, 64), (3, 131, 203), (16, 1080, 1920), (5, 96, 136))
DEHAZING = ((SIX, 1), (SIX, 2), (SIX, 3), (DICT, 0), (DICT, 1), (DICT, 2))
CODE_DOMAIN = ((SIX, 5), (DICT, 3))  # one code-domain strategy per surface
VARIANTS = {
    "gf_exact": {"gf_exact": 1},
    "fx32": {"inter_dtype": _lib.INTER_FX32},
    "f32t": {"inter_dtype": _lib.INTER_F32T},
    "dark_patch7": {"dark_patch": 7},
    "no_cast": {"cast_correct": 0},
    "forced_cast": {"forced_cast": 1},
    "min_size2048": {"min_size": 2048},
    "tiles1x1": {"tiles_x": 1, "tiles_y": 1},
    "tiles16x16": {"tiles_x": 16, "tiles_y": 16},
    "gf_ksize1": {"gf_ksize": 1},
    "gf_ksize64": {"gf_ksize": 64},
}

# sizes under a context's tuning (uwie_workspace_bytes_ctx)
CTX_SHAPES = ((5, 96, 136), (16, 1080, 1920))
CTX_SETS = ((SIX, 1), (SIX, 2), (SIX, 3), (DICT, 0))
CTX_TUNINGS = {
    "default": {},
    "restore_store": {"restore_store": 1},
    "select_generic": {"select_generic": 1},
    "entry_fuse0": {"entry_fuse": 0},
    "entry_fuse2": {"entry_fuse": 2},
    "q_hist0": {"q_hist": 0},
    "streams2": {"streams": 2},
    "streams3": {"streams": 3},
    "streams4": {"streams": 4},
}


def params(lib, surface, strategy, **over):
    p = _lib.UwieParams()
    assert lib.uwie_params_init(ctypes.byref(p), surface, strategy) == 0
    for key, value in over.items():
        assert hasattr(p, key), key
        setattr(p, key, value)
    return p


def name_of(surface, strategy):
    return f"{'six' if surface == SIX else 'dict'}{strategy}"


def array_of(sets):
    arr = (_lib.UwieParams * len(sets))()
    for i, p in enumerate(sets):
        arr[i] = p
    return arr


def six_set(lib, exact3=False):
    """The six six_stadigy sets of uwie_enhance_all_u8; exact3: only strategy 3 asks for the exact-order guided filter."""
    return array_of([params(lib, SIX, k + 1, **({"gf_exact": 1} if exact3 and k == 2 else {})) for k in range(6)])


def mixed_list(lib):
    """uwie_select_best_u8's list with both surfaces, both kinds of pipeline and two stored-image layouts."""
    return array_of([params(lib, SIX, 2), params(lib, DICT, 0), params(lib, DICT, 3), params(lib, SIX, 3)])


def cpu_sizes(lib):
    """name -> [bytes at each of SHAPES] of every sizing function that needs no context."""
    out = {}

    def at_shapes(fn):
        return [int(fn(B, H, W)) for B, H, W in SHAPES]

    for surface, strategy in DEHAZING + CODE_DOMAIN:
        for vname, over in VARIANTS.items():
            p = params(lib, surface, strategy, **over)
            out[f"{name_of(surface, strategy)}/{vname}"] = at_shapes(lambda B, H, W: lib.uwie_workspace_bytes(B, H, W, ctypes.byref(p)))
    out["all/null"] = at_shapes(lambda B, H, W: lib.uwie_workspace_bytes_all(B, H, W, None))
    p6 = six_set(lib, exact3=True)
    out["all/exact3"] = at_shapes(lambda B, H, W: lib.uwie_workspace_bytes_all(B, H, W, ctypes.cast(p6, ctypes.c_void_p)))
    ps = mixed_list(lib)
    for with_outputs in (0, 1):
        out[f"select/with_outputs{with_outputs}"] = at_shapes(
            lambda B, H, W: lib.uwie_workspace_bytes_select(B, H, W, ctypes.cast(ps, ctypes.c_void_p), len(ps), with_outputs))
    for surface, strategy in ((SIX, 2), (DICT, 0)):
        p = params(lib, surface, strategy)
        for elem in (4, 8):
            out[f"float{elem}/{name_of(surface, strategy)}"] = at_shapes(
                lambda B, H, W: lib.uwie_workspace_bytes_float(B, H, W, ctypes.byref(p), elem))
    return out


def ctx_sizes(dev):
    """name -> [bytes at each of CTX_SHAPES] of uwie_workspace_bytes_ctx under each of CTX_TUNINGS.  No kernel is launched."""
    out = {}
    for tname, tune in CTX_TUNINGS.items():
        with dev.tuning(**tune):
            for surface, strategy in CTX_SETS:
                p = params(dev.lib, surface, strategy)
                out[f"{name_of(surface, strategy)}/{tname}"] = [
                    int(dev.lib.uwie_workspace_bytes_ctx(dev._ctx, B, H, W, ctypes.byref(p))) for B, H, W in CTX_SHAPES]
    return out


def recorded(section):
    with open(GOLDEN) as f:
        return json.load(f)[section]
