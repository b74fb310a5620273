"""Generate tests/golden/train_batches.npz: items of the REAL reference datasets and predictor preprocessing.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
deep_learning_parameters, vgg_16_UIE and use_trained_model are imported with stand-ins: ``cv2`` is tests/resize_ref.py's
resize for the RGB frames plus tests/gen_golden_features79.py's primitives (its ``resize128`` for FeatureExtractor's gray
128x128 resize, the contract of the existing feature kernels) (``imread`` returns the fixture frames in BGR by file name,
``cvtColor(BGR2RGB)`` reverses the channels) and ``torchvision.transforms.Normalize`` is the float32 ``sub`` / ``div``.
What the fixture pins is the reference's own glue: BGR -> RGB, resize before ``/ 255``, the flip order and the order of
the ``np.random`` draws, which image the features are taken from, dtypes and shapes.

Stored (only arrays travel):
* ``frame_<name>``: the input frames (RGB u8), except the 1080p one, which is ``resize_ref.synth_frame(1080, 1920, 77)``;
* ``<group>/image``, ``<group>/reference``: the items' float32 tensors stored as u8 (asserted equal to ``u8 / 255``;
  ``reference`` only for the items whose reference exists, the others' is asserted equal to the image),
  ``<group>/features``: float32 rows, ``<group>/names``, ``<group>/refs``, ``<group>/size``, ``<group>/seed``;
* ``vgg/<name>``: ``_preprocess_for_vgg`` float32 ``[1,3,s,s]``; ``tensor/<name>``: ``_img_to_tensor`` float32.

Run:  python tests/gen_golden_train_batches.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
import gen_golden_features79 as gf  # noqa: E402
import resize_ref as RR  # noqa: E402

OUT = os.path.join(HERE, "golden", "train_batches.npz")
BIG = ("hd_1080x1920", 1080, 1920, 77)


def frames():
    """name -> RGB u8 frame: odd, 2x the 64 target, smaller than the targets, one wide, one 1080p."""
    out = {
        "odd_37x53": RR.synth_frame(37, 53, 1),
        "area_128x128": RR.synth_frame(128, 128, 2),
        "small_30x20": RR.synth_frame(30, 20, 3),
        "wide_90x160": RR.synth_frame(90, 160, 4),
        "tall_151x67": RR.synth_frame(151, 67, 5),
    }
    name, h, w, seed = BIG
    out[name] = RR.synth_frame(h, w, seed)
    return out


# references on disk: the same names in the reference folder; a missing one -> ref = img.copy()
REFS = {"odd_37x53": (41, 50, 11), "area_128x128": (100, 90, 12), "wide_90x160": (45, 80, 14), "tall_151x67": (160, 70, 15)}


def stand_ins():
    mods = gf.stand_ins()
    cv2 = mods["cv2"]
    cv2.COLOR_BGR2RGB, cv2.INTER_LINEAR = "bgr2rgb", 1
    cvt = cv2.cvtColor
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1]) if code == "bgr2rgb" else cvt(img, code)

    gray128 = cv2.resize  # feature_extraction's GLCM resize: features79_ref.resize128, the merged kernel's contract

    def resize(img, dsize, interpolation=1):
        assert interpolation == 1 and img.dtype == np.uint8
        return gray128(img, dsize) if img.ndim == 2 else RR.resize(img, dsize)

    cv2.resize = resize
    tv = types.ModuleType("torchvision")
    tv.__path__ = []
    tr = types.ModuleType("torchvision.transforms")

    class Normalize:
        def __init__(self, mean, std):
            import torch
            self.mean = torch.as_tensor(mean, dtype=torch.float32)[:, None, None]
            self.std = torch.as_tensor(std, dtype=torch.float32)[:, None, None]

        def __call__(self, t):
            return t.clone().sub_(self.mean).div_(self.std)

    tr.Normalize = Normalize
    tv.transforms, tv.models = tr, gg._Inert("torchvision.models")
    mods.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.models": tv.models})
    return mods


def as_u8(t):
    a = t.numpy()
    u8 = np.rint(a * 255).astype(np.uint8)
    assert a.dtype == np.float32 and np.array_equal(u8.astype(np.float32) / np.float32(255.0), a)
    return np.ascontiguousarray(np.moveaxis(u8, 0, -1))


def main():
    fr = frames()
    refs = {k: RR.synth_frame(*v) for k, v in REFS.items()}
    sys.dont_write_bytecode = True
    with tempfile.TemporaryDirectory() as tmp:
        img_dir, ref_dir = Path(tmp, "img"), Path(tmp, "ref")
        img_dir.mkdir(), ref_dir.mkdir()
        for k in fr:
            (img_dir / f"{k}.png").touch()
        for k in refs:
            (ref_dir / f"{k}.png").touch()
        for name, m in stand_ins().items():
            sys.modules[name] = m
        sys.path.insert(0, gg.REF)
        import deep_learning_parameters as D
        import feature_extraction as FE
        import use_trained_model as U
        import vgg_16_UIE as V
        sys.path.remove(gg.REF)

        def read(path):  # imread: the fixture frame of that name, in BGR; the reference folder holds other frames
            p = Path(path)
            return np.ascontiguousarray((refs if p.parent == ref_dir else fr)[p.stem][:, :, ::-1])

        sys.modules["cv2"].imread = read
        out = {}
        for k, f in fr.items():
            if k != BIG[0]:
                out["frame_" + k] = f
        for k, f in refs.items():
            out["ref_" + k] = f

        def record(group, ds, names, seed=None):
            ds.image_paths = [img_dir / f"{n}.png" for n in names]
            if seed is not None:
                np.random.seed(seed)
            items = []
            with contextlib.redirect_stdout(io.StringIO()):
                for i in range(len(names)):
                    items.append(ds[i])
            out[f"{group}/names"] = np.array(names)
            out[f"{group}/refs"] = np.array([n in refs for n in names])
            out[f"{group}/size"] = np.array(ds.target_size)
            out[f"{group}/seed"] = np.array(-1 if seed is None else seed)
            out[f"{group}/image"] = np.stack([as_u8(it["image"]) for it in items])
            for it, n in zip(items, names):  # a missing reference is the image (asserted); only the others are stored
                if n not in refs:
                    assert np.array_equal(it["reference"].numpy(), it["image"].numpy())
            sz = ds.target_size
            out[f"{group}/reference"] = np.array([as_u8(it["reference"]) for it, n in zip(items, names) if n in refs],
                                                 np.uint8).reshape(-1, sz, sz, 3)
            feats = np.stack([it["features"].numpy() for it in items])
            assert feats.dtype == np.float32
            out[f"{group}/features"] = feats
            print(f"{group}: {len(items)} items at {ds.target_size}, features {feats.shape}")
            return items

        # EnhancementDataset (EndToEndTrainer): FeatureExtractor of the resized float image
        small = ["odd_37x53", "area_128x128", "small_30x20", "wide_90x160", "tall_151x67"]
        ds = D.EnhancementDataset(img_dir, ref_dir, FE.FeatureExtractor(), target_size=64)
        record("dlp64", ds, small)
        ds = D.EnhancementDataset(img_dir, ref_dir, FE.FeatureExtractor(), target_size=256)
        record("dlp256", ds, [BIG[0]])
        # ImprovedEnhancementDataset (ImprovedTrainer): augment_pair's flips, extract_basic_features of the flipped image
        seed = next(s for s in range(1000) if len({(a > 0.5, b > 0.5) for a, b in np.random.RandomState(s).rand(5, 2)}) == 4)
        ds = V.ImprovedEnhancementDataset.__new__(V.ImprovedEnhancementDataset)
        ds.reference_folder, ds.target_size, ds.augment, ds.use_features = ref_dir, 40, True, True
        record("vgg40", ds, small, seed=seed)
        ds = V.ImprovedEnhancementDataset.__new__(V.ImprovedEnhancementDataset)
        ds.reference_folder, ds.target_size, ds.augment, ds.use_features = ref_dir, 112, True, True
        record("vgg112", ds, [BIG[0]], seed=seed + 1)
        ds = V.ImprovedEnhancementDataset.__new__(V.ImprovedEnhancementDataset)
        ds.reference_folder, ds.target_size, ds.augment, ds.use_features = ref_dir, 40, False, False
        record("vgg40_plain", ds, small[:2])
        # EnhancementPredictor: _preprocess_for_vgg and _img_to_tensor of the float image u8 / 255
        pred = U.EnhancementPredictor.__new__(U.EnhancementPredictor)
        import torchvision.transforms as T
        pred.normalize = T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
        for name, size in (("odd_37x53", 56), (BIG[0], 56), ("area_128x128", 64)):
            pred.input_size = size
            img = fr[name].astype(np.float32) / 255.0
            out[f"vgg/{name}"] = pred._preprocess_for_vgg(img).numpy()
            out[f"vgg/{name}/size"] = np.array(size)
        for name in ("odd_37x53", "small_30x20"):
            img = fr[name].astype(np.float32) / 255.0
            out[f"tensor/{name}"] = pred._img_to_tensor(img).numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; vgg40 seed", seed)


if __name__ == "__main__":
    main()
