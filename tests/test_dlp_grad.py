"""CPU checks of the gated-gamma DifferentiableEnhancement (deep_learning_parameters.py:24-90): the C ABI of its four entry
points, the host's replay of the reference's indexing errors, and the torch-CPU restatement (tests/dlp_grad_ref.py) against
the real module's gradients (tests/golden/dlp_grads.npz)."""
import os

import numpy as np
import pytest

import dlp_grad_ref as R
import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd import _lib
from underwater_image_enhancement_amd.api import _raise_rank_error

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlp_grads.npz")
NEW = ("uwie_diff_gated_f32", "uwie_diff_gated_save_f32", "uwie_diff_gated_bwd_f32", "uwie_diff_gated_bwd_workspace_bytes")
CASES = ("u8ties_2x3x24x31", "rand_3x3x17x40", "flat_1x3x8x8", "use0_2x3x13x19", "use1_2x3x11x23", "use037_2x3x12x15",
         "usemix_4x3x10x9", "gammain_2x3x14x16", "gammaout_3x3x9x21", "sameL_2x3x9x14", "khilast_1x3x10x12", "negL_2x3x10x12",
         "predictor_3x3x32x32", "px_2x3x1x1", "row_1x3x1x37")
ERRORS = (IndexError, ValueError, OverflowError)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return uw.load()


def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def test_gated_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert uw.GatedDifferentiableEnhancement and uw.GatedDiffEnhanceFunction


def test_gated_entry_points_reject_null_arguments_without_a_gpu(lib):
    assert lib.uwie_diff_gated_f32(None, None, None, 1, 8, 8, 1, None, 0, None, 0, None) == -1
    assert b"NULL" in lib.uwie_last_error()
    assert lib.uwie_diff_gated_save_f32(None, None, None, 1, 8, 8, 1, None, 0, None, None, 0, None) == -1
    assert b"NULL" in lib.uwie_last_error()
    assert lib.uwie_diff_gated_bwd_f32(None, None, None, 0, 1, 1, 8, 8, None, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.uwie_last_error()


def test_gated_backward_workspace_is_the_vgg_one(lib):
    for B, H, W in ((1, 1, 1), (4, 256, 256), (32, 224, 224), (8, 2160, 3840), (3, 211, 157)):
        need = lib.uwie_diff_gated_bwd_workspace_bytes(B, H, W)
        assert need == lib.uwie_diff_enhance_bwd_workspace_bytes(B, H, W)
        assert 0 < need <= lib.uwie_workspace_bytes(B, H, W, None)
    assert lib.uwie_diff_gated_bwd_workspace_bytes(0, 8, 8) == 0


def test_missing_key_raises_key_error_before_touching_the_device():
    img = np.zeros((1, 3, 4, 4), np.float32)
    full = {"L_low": [[5.0]], "L_high": [[95.0]], "use_gamma": [[0.5]], "gamma": [[1.2]]}
    for key in full:
        with pytest.raises(KeyError, match=key):
            uw.GatedDifferentiableEnhancement()(img, {k: v for k, v in full.items() if k != key})


def test_golden_file_covers_the_contract_cases():
    cases = golden()
    assert set(CASES) <= set(cases), sorted(set(CASES) - set(cases))
    for tag in CASES:
        c = cases[tag]
        assert c["grad_img"].shape == c["img"].shape == c["grad_img_stable"].shape, tag
        assert c["grad_use_gamma"].shape == c["grad_gamma"].shape == (c["img"].shape[0], 1), tag
    src = cases["u8ties_2x3x24x31"]["src"]
    assert np.any(src[:, :, :2] != src[:, :, 2:])
    for tag in ("rand_3x3x17x40", "predictor_3x3x32x32", "use037_2x3x12x15"):
        assert np.array_equal(cases[tag]["grad_img"], cases[tag]["grad_img_stable"]), tag
    assert not cases["use0_2x3x13x19"]["use_gamma"].any() and (cases["use1_2x3x11x23"]["use_gamma"] == 1).all()
    assert set(np.unique(cases["usemix_4x3x10x9"]["use_gamma"])) >= {0.0, 1.0, np.float32(0.37)}
    g_in, g_out = cases["gammain_2x3x14x16"]["gamma"], cases["gammaout_3x3x9x21"]["gamma"]
    assert ((g_in >= 1) & (g_in <= 1.5)).all() and ((g_out < 1) | (g_out > 1.5)).any()
    c = cases["sameL_2x3x9x14"]
    assert np.array_equal(c["L_low"], c["L_high"])
    c = cases["khilast_1x3x10x12"]
    assert (c["k"][:, 1] == c["img"].shape[2] * c["img"].shape[3] - 1).all()
    c = cases["negL_2x3x10x12"]
    n = c["img"].shape[2] * c["img"].shape[3]
    assert (c["L_low"] < 0).all() and c["k"][0, 0] == n - 3 and c["k"][1, 0] == 0
    c = cases["predictor_3x3x32x32"]
    assert ((c["L_low"] >= 5) & (c["L_low"] <= 20)).all() and ((c["L_high"] >= 85) & (c["L_high"] <= 98)).all()
    assert np.isnan(cases["errors"]["L"]).any() and np.isinf(cases["errors"]["L"]).any()
    assert set(cases["errors"]["code"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_the_module(tag):
    c = golden()[tag]
    out, gi, gu, gg = R.grads(c["img"], c["L_low"], c["L_high"], c["use_gamma"], c["gamma"], c["grad_out"])
    assert np.array_equal(out, c["out"]), f"{tag}: forward differs"
    n = c["img"].shape[2] * c["img"].shape[3]
    assert np.array_equal(np.stack([R.sorted_positions(c["L_low"], n), R.sorted_positions(c["L_high"], n)], axis=1), c["k"])
    want = {"grad_img": c["grad_img_stable"], "grad_use_gamma": c["grad_use_gamma"], "grad_gamma": c["grad_gamma"]}
    got = {"grad_img": gi, "grad_use_gamma": gu, "grad_gamma": gg}
    worst = R.check_grads(c["img"], c["L_low"], c["L_high"], c["grad_out"], got, want, tag=tag)
    print(f"{tag}: worst grad_img error {worst:.3f} of the bound")


def test_host_replays_the_modules_exceptions():
    e = golden()["errors"]
    n = int(e["n"])
    for L, code in zip(e["L"], e["code"]):
        with pytest.raises(ERRORS[code]):
            _raise_rank_error(L[None], n)
    _raise_rank_error(np.array([[5.0, 95.0], [-100.0, 99.9]], np.float32), n)  # valid: no exception
