"""Host-side pieces of the loss-map outputs (loss_map_outputs.py, stage1.py --loss_maps) on a stubbed handle: no GPU needed."""
import os
import types

import numpy as np
import pytest

H, W, F = 5, 7, 3


class _StubHandle:
    """The AtlasFit surface evaluate_model_single / write_loss_maps use, with deterministic maps."""

    def __init__(self, two_layer):
        self.two_layer = two_layer
        self.cfg = types.SimpleNamespace(number_of_frames=F, resx=W, resy=H)
        self.calls = []

    def render_frame(self, f):
        return np.full((H, W, 3), 0.25 * (f + 1), np.float32), 1.0

    def loss_maps(self, f, which=None):
        self.calls.append(("loss_maps", f, which))
        rng = np.random.default_rng(f)
        names = ("rigidity_loss1", "flow_loss1", "rgb_error", "rgb_residual") + (("rigidity_loss2", "flow_loss2", "flow_alpha_loss") if self.two_layer else ())
        out = {k: rng.uniform(0, 2, (H, W)).astype(np.float32) for k in names}
        out["rgb_residual"] = rng.uniform(-0.7, 0.7, (H, W, 3)).astype(np.float32)
        return out

    def render_layers(self, f):
        u = np.linspace(-1, 1, H * W * 2, dtype=np.float32).reshape(H, W, 2)
        return {"uv1": u, "alpha": np.full((H, W), 0.5 + 0.1 * f, np.float32)}


def test_casts_follow_the_reference():
    from aiod_amd.loss_map_outputs import alpha_vs_mask, residual_u8, uv1_masked
    r = np.array([[-0.5, 0.0, 0.499999, 0.5, -0.2]], np.float32)
    assert residual_u8(r).tolist() == ((r.astype(np.float64) + 0.5) * 255).astype(np.uint8).tolist() == [[0, 127, 254, 255, 76]]
    uv = np.array([[[-1.0, 1.0], [0.2, -0.4]]], np.float32)
    m = uv1_masked(uv, np.array([[1.0, 0.5]], np.float32))
    assert m.shape == (1, 2, 3) and m[0, :, 0].tolist() == [0, 76] and m[0, :, 1].tolist() == [255, 38] and (m[:, :, 2] == 0).all()
    av = alpha_vs_mask(np.array([[1.0, 0.0]]), np.array([[0.5, 0.999]], np.float32))
    assert av[0].tolist() == [[255, 127, 0], [0, 254, 0]]


def _tree(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


@pytest.mark.parametrize("two_layer", [False, True])
def test_cli_flag_file_tree(tmp_path, two_layer):
    from PIL import Image
    from aiod_amd import stage1 as S
    from aiod_amd.loss_map_outputs import residual_u8
    video = np.zeros((H, W, 3, F), np.float32)
    masks = np.stack([np.eye(H, W) * (f + 1) / F for f in range(F)], axis=2).astype(np.float32)
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    af = _StubHandle(two_layer)
    S.evaluate_model_single(af, video, plain, 10, save_checkpoint_file=False)
    assert af.calls == []                                           # without the flag no map is computed
    assert [p for p in _tree(plain) if not p.startswith("000010/PSNR_")] == ["output/%05d.png" % f for f in range(F)]
    S.evaluate_model_single(af, video, flagged, 10, save_checkpoint_file=False, loss_maps=True, mask_frames=masks)
    extra = sorted(set(_tree(flagged)) - set(_tree(plain)))
    dirs = ("alpha_vs_mask", "residuals", "uv_1_masked") if two_layer else ("residuals",)
    assert extra == sorted(["000010/loss_maps.npz"] + ["000010/%s/%05d.png" % (d, f) for d in dirs for f in range(F)])
    assert set(_tree(plain)) <= set(_tree(flagged))
    z = dict(np.load(flagged / "000010" / "loss_maps.npz"))
    ref = [af.loss_maps(f) for f in range(F)]
    assert sorted(z) == sorted(ref[0])
    for k in z:
        assert z[k].dtype == np.float32 and np.array_equal(z[k], np.stack([r[k] for r in ref]))
    for f in range(F):
        png = np.asarray(Image.open(flagged / "000010" / "residuals" / ("%05d.png" % f)))
        assert np.array_equal(png, residual_u8(ref[f]["rgb_residual"]))
    if two_layer:
        av = np.asarray(Image.open(flagged / "000010" / "alpha_vs_mask" / "00002.png"))
        assert av.shape == (H, W, 3) and av[0, 0].tolist() == [255, int(0.7 * 255), 0]


def test_fg_bg_needs_masks(tmp_path):
    from aiod_amd.loss_map_outputs import write_loss_maps
    with pytest.raises(ValueError):
        write_loss_maps(_StubHandle(True), str(tmp_path))


def test_cli_flag_is_registered_and_off_by_default():
    import argparse
    from aiod_amd import stage1 as S
    seen = {}
    orig = argparse.ArgumentParser.parse_args

    def grab(self, argv=None, namespace=None):
        ns = orig(self, argv, namespace)
        seen.update(vars(ns))
        raise SystemExit(0)
    argparse.ArgumentParser.parse_args = grab
    try:
        for two in (False, True):
            for argv, want in (([], False), (["--loss_maps"], True)):
                seen.clear()
                with pytest.raises(SystemExit):
                    S._cli(argv, two_layer=two)
                assert seen["loss_maps"] is want, (two, argv)
    finally:
        argparse.ArgumentParser.parse_args = orig
