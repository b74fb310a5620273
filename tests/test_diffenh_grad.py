"""CPU checks of DifferentiableEnhancement's backward: the C ABI of the two new entry points, and the torch-CPU restatement
(tests/diffenh_grad_ref.py) against the real module's gradients (tests/golden/vgg_grads.npz)."""
import os

import numpy as np
import pytest

import diffenh_grad_ref as R
import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgg_grads.npz")
NEW = ("uwie_diff_enhance_save_f32", "uwie_diff_enhance_bwd_f32", "uwie_diff_enhance_bwd_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return uw.load()


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def test_backward_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_backward_entry_points_reject_null_arguments_without_a_gpu(lib):
    assert lib.uwie_diff_enhance_save_f32(None, None, None, 1, 8, 8, 1, None, 3, None, None, 0, None) == -1
    assert lib.uwie_diff_enhance_bwd_f32(None, None, None, 3, 1, 1, 8, 8, None, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.uwie_last_error()


def test_backward_workspace_is_small_and_within_the_stage_workspace(lib):
    for B, H, W in ((1, 1, 1), (8, 224, 224), (32, 224, 224), (8, 2160, 3840), (3, 211, 157)):
        need = lib.uwie_diff_enhance_bwd_workspace_bytes(B, H, W)
        assert 0 < need <= B * 64 * 1024 + 512
        assert need <= lib.uwie_workspace_bytes(B, H, W, None)
    assert lib.uwie_diff_enhance_bwd_workspace_bytes(0, 8, 8) == 0


def test_golden_file_covers_the_contract_cases():
    cases = golden_cases()
    assert len(cases) >= 11
    for tag, c in cases.items():
        assert bool(c["L_grad_is_none"]), tag
        assert c["grad_img"].shape == c["img"].shape == c["grad_img_stable"].shape, tag
    # ties: torch's default sort and the stable rule pick different elements in some planes; elsewhere the two agree
    src = cases["u8ties_2x3x24x31"]["src"]
    assert np.any(src[:, :, :2] != src[:, :, 2:])
    for tag in ("rand_3x3x17x40", "dark_1x3x33x21", "stretch_2x3x16x16"):
        assert np.array_equal(cases[tag]["grad_img"], cases[tag]["grad_img_stable"]), tag


@pytest.mark.parametrize("tag", sorted(golden_cases()))
def test_restatement_matches_the_module(tag):
    c = golden_cases()[tag]
    out, gi, gom, gga = R.grads(c["img"], c["L_low"], c["L_high"], c.get("omega"), c.get("gamma"), c["grad_out"])
    assert np.array_equal(out, c["out"]), f"{tag}: forward differs"
    want = {"grad_img": c["grad_img_stable"]}
    got = {"grad_img": gi}
    for key, v in (("grad_omega", gom), ("grad_gamma", gga)):
        if key in c:
            want[key], got[key] = c[key], v
    worst = R.check_grads(c["img"], c["L_low"], c["L_high"], c["grad_out"], got, want, tag=tag)
    print(f"{tag}: worst grad_img error {worst:.3f} of the bound")
