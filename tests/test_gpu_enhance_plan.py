"""The workspace contract of the enhance entry points: the size functions answer for a parameter set, a shape and a context's
tuning, and a call on exactly that many bytes stays inside them, finds its percentiles there again and gives the bytes of a
call on the Device's ordinary workspace -- on every pipeline, selection route and layout that plan_enhance can choose."""
import ctypes
import re

import numpy as np
import pytest

import workspace_cases as wc
from test_gpu_dark_patch import e2e_frames

pytestmark = pytest.mark.gpu

SIX, DICT = wc.SIX, wc.DICT
E_WORKSPACE = -2  # include/uwie.h UWIE_E_WORKSPACE
GUARD = 1 << 20
H, W = 96, 136

SETS = ((SIX, 1), (SIX, 2), (SIX, 3), (SIX, 5), (DICT, 0), (DICT, 3))  # dict: strong_dehazing, clahe_enhancement
TUNINGS = ({}, {"restore_store": 1}, {"select_generic": 1}, {"entry_fuse": 0}, {"entry_fuse": 1}, {"entry_fuse": 2}, {"streams": 3},
           {"gf_fuse": 1})
# parameter variants (default tuning): the exact-order filter's planes, k_trans_patch's t0 plane, float32 t, and a leaf size
# at which cast detection's chunk pass does not feed the quadtree
VARIANTS = ({"gf_exact": 1}, {"dark_patch": 15}, {"inter_dtype": 2}, {"min_size": 2048})


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    d = uw.get_device(0)
    yield d
    assert d.check_status() == 0


@pytest.fixture(scope="module")
def batches(dev):
    """batch -> u8 device tensor [batch, 96, 136, 3]: noise_96x136 and four rearrangements of it."""
    u8 = e2e_frames()["noise_96x136"]
    five = np.stack([u8, u8[::-1], u8[:, ::-1], np.roll(u8, 17, axis=1), u8[..., ::-1]])
    return {1: dev.tensor(u8[None]), 5: dev.tensor(five)}


def test_sizes_under_tuning_are_unchanged(dev):
    """uwie_workspace_bytes_ctx under every tuning that moves a buffer or splits the batch: no kernel is launched."""
    want, got = wc.recorded("context"), wc.ctx_sizes(dev)
    assert sorted(got) == sorted(want) and len(got) == len(wc.CTX_SETS) * len(wc.CTX_TUNINGS)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


class Guarded:
    """A buffer of `need` bytes followed by a guard MiB of 0xA5 that no call may touch."""

    def __init__(self, dev, need):
        import torch

        self.need = need
        self.buf = torch.empty(need + GUARD, dtype=torch.uint8, device=dev.torch_device)
        self.buf[need:] = 0xA5
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.need:] == 0xA5).all().item())


def needed_by_the_call(dev, call):
    """The bytes the call itself requires: what its 'workspace too small' message names when it is given 256."""
    assert call(256) == E_WORKSPACE
    m = re.search(rb"workspace too small: need (\d+) bytes, got 256", dev.lib.uwie_last_error())
    assert m, dev.lib.uwie_last_error()
    return int(m.group(1))


def launches_nothing(dev, short_call, what):
    dev.profile(True)
    try:
        dev.profile_rows()
        assert short_call() == E_WORKSPACE, what
        assert b"workspace too small" in dev.lib.uwie_last_error(), what
        assert dev.profile_rows() == {}, what
    finally:
        dev.profile(False)


def check_cell(dev, frames, p, what):
    import torch

    from underwater_image_enhancement_amd.runtime import _ptr

    B = int(frames.shape[0])
    dehazing = (p.surface == SIX and p.strategy <= 3) or (p.surface == DICT and p.strategy <= 2)
    if dehazing:
        want, _, want_pct = dev.enhance_u8_with_percentiles(frames, p)
    else:
        want = dev.enhance_u8(frames, p)[0]
    need = dev.lib.uwie_workspace_bytes_ctx(dev._ctx, B, H, W, ctypes.byref(p))
    ws = Guarded(dev, need)
    out = dev.empty((B, H, W, 3), torch.uint8)

    def call(nbytes):
        return dev.lib.uwie_enhance_u8(dev._ctx, _ptr(frames), _ptr(out), None, B, H, W, ctypes.byref(p), ws.ptr, nbytes, dev.stream())

    assert call(need) == 0, what
    assert torch.equal(out, want), what
    if dehazing:
        pct = dev.empty(tuple(want_pct.shape), torch.float64)
        assert dev.lib.uwie_enhance_percentiles(dev._ctx, ws.ptr, need, B, H, W, ctypes.byref(p), _ptr(pct), dev.stream()) == 0, what
        assert torch.equal(pct, want_pct), what
    assert ws.intact(), what
    # 256 bytes less than the call requires: UWIE_E_WORKSPACE and nothing launched.  What it requires is the whole batch's
    # layout; uwie_workspace_bytes_ctx also covers every sub-batch split (each slice has its own fixed-size selection
    # buffers), so the two agree for a batch that cannot be split and the call's share is the smaller one otherwise.
    required = needed_by_the_call(dev, call)
    assert required == need if B == 1 else required <= need, (what, required, need)
    launches_nothing(dev, lambda: call(required - 256), what)


def all_call(dev, frames, p6, out, ws, nbytes):
    from underwater_image_enhancement_amd.runtime import _ptr

    return dev.lib.uwie_enhance_all_u8(dev._ctx, _ptr(frames), _ptr(out), None, int(frames.shape[0]), H, W,
                                       ctypes.cast(p6, ctypes.c_void_p), ws.ptr, nbytes, dev.stream())


def test_the_plans_layout_is_sufficient_and_self_contained(dev, batches):
    import torch

    for B, frames in batches.items():
        for surface, strategy in SETS:
            dz = (surface, strategy) in wc.DEHAZING
            cells = [(tune, {}) for tune in TUNINGS] + [({}, over) for over in VARIANTS if dz]
            for tune, over in cells:
                with dev.tuning(**tune):
                    check_cell(dev, frames, wc.params(dev.lib, surface, strategy, **over), (B, wc.name_of(surface, strategy), tune, over))
        # the fan-out on uwie_workspace_bytes_all's bytes: the default six sets, and a layout that only strategy 3's
        # exact-order filter gives its planes
        for exact3 in (False, True):
            p6 = wc.six_set(dev.lib, exact3)
            need = dev.lib.uwie_workspace_bytes_all(B, H, W, ctypes.cast(p6, ctypes.c_void_p))
            ws = Guarded(dev, need)
            out = dev.empty((6, B, H, W, 3), torch.uint8)
            for tune in TUNINGS:
                with dev.tuning(**tune):
                    singles = torch.stack([dev.enhance_u8(frames, p6[k])[0] for k in range(6)])
                    out.zero_()
                    assert all_call(dev, frames, p6, out, ws, need) == 0, (B, exact3, tune)
                    assert torch.equal(out, singles), (B, exact3, tune)
            assert ws.intact(), (B, exact3)
            # (uwie_workspace_bytes_all knows no context: it is exact for the default tuning)
            assert needed_by_the_call(dev, lambda n: all_call(dev, frames, p6, out, ws, n)) == need
            launches_nothing(dev, lambda: all_call(dev, frames, p6, out, ws, need - 256), (B, exact3))
