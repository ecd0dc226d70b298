"""Stage 2's precision mode "fp16" on the GPU (include/atlasfit.h: AF_FILTER_FP16, af_filter_set_precision, af_conv2d_prec;
csrc/conv_gemm_h.h with REFLECT, k_conv_h): both nets as the reference's modules compute them under fp16 autocast.

Yardsticks, the rules of tests/test_gpu_raft_fp16.py.  The "contract twin" is tests/stage2_fp16_ref.py in fp64: the mode's rounding
contract with exact sums.  A single layer is held against it tightly: the kernel accumulates exact products in fp32,
so it can differ from the twin only where the fp32 sum and the fp64 sum round to different fp16 values, on at most 1 % of the outputs
(tests/test_stage2_fp16_host.py: an fp32-accumulating restatement differs on 0.06 - 0.29 % of these shapes' outputs, torch's own half
convolution on 0.05 - 0.44 %); the difference is bounded by twice torch's half convolution on the same operands, or one fp16 ulp at the
largest output.  The end-to-end tensors are held against the fp64 twin of tests/golden/stage2.npz with the project's usual rule, at
most twice the error of the reference's own modules under fp16 autocast (tests/golden/stage2_amp.npz)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage2_fp16_ref as S16  # noqa: E402
from test_gpu_raft_fp16 import stats, is_fp16_valued  # noqa: E402
from test_gpu_stage2 import g2, ref_loop, _frames  # noqa: E402,F401

ACTS = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec4", "dec3", "dec2", "dec1", "E3", "RB")


def hwc(t):
    return t[0].permute(1, 2, 0).contiguous()


def gpu_conv(x, wt, b, r, shape, act, precision="fp16"):
    from aiod_amd.stage2 import conv2d
    return conv2d(hwc(x).numpy(), wt.numpy(), None if b is None else b.numpy(), shape[3], shape[4], act, None if r is None else hwc(r).numpy(),
                  precision=precision)


def conv_case(name, shape, act, x, wt, b, r=None):
    """The conditions of a single convolution (tests/test_gpu_raft_fp16.py::conv_case); prints every figure before it asserts."""
    d = lambda t: None if t is None else t.double()      # noqa: E731
    twin = hwc(S16.conv2d(d(x), d(wt), d(b), shape[3], shape[4], act, d(r))).numpy()
    th = hwc(S16.torch_half_conv(x, wt, b, shape[3], shape[4], act, r)).numpy()
    y = gpu_conv(x, wt, b, r, shape, act)
    assert y.shape == twin.shape and np.isfinite(y).all() and is_fp16_valued(y)
    frac = float((y.astype(np.float64) != twin).mean())
    hm, hr = stats(y, twin)
    tm, tr = stats(th, twin)
    ulp = float(np.spacing(np.float16(np.abs(twin).max())))
    print("%-44s differ %.4f %% | hip max %.3e rms %.3e | torch half max %.3e rms %.3e (differ %.4f %%) | ulp at max %.3e"
          % (name, 100 * frac, hm, hr, tm, tr, 100 * float((th != twin).mean()), ulp))
    assert frac <= 0.01, "%s: %.3f %% of the outputs differ from the twin's fp16 value" % (name, 100 * frac)
    assert hm <= max(2.0 * tm, ulp), "%s: max |hip - twin| %.3e > max(2 x %.3e, %.3e)" % (name, hm, tm, ulp)
    assert hr <= 2.0 * tr, "%s: rms |hip - twin| %.3e > 2 x %.3e" % (name, hr, tr)
    return y


# ---- single convolutions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=S16.ACT_NAMES)
@pytest.mark.parametrize("shape", S16.SWEEP, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_against_the_contract_twin(shape, act):
    conv_case("conv %s %s" % (shape, S16.ACT_NAMES[act]), shape, act, *S16.draw_conv(shape))


def test_conv_with_a_residual():
    shape = S16.SWEEP[1]                  # the ResidualBlock's second convolution: no activation, + x
    conv_case("conv %s none + residual" % (shape,), shape, 0, *S16.draw_conv(shape, residual=True))
    conv_case("conv %s leaky + residual" % (shape,), shape, 2, *S16.draw_conv(shape, residual=True))


def test_reflection_equals_zero_padding_of_the_reflected_input():
    shape = S16.SWEEP[0]
    x, wt, b, _ = S16.draw_conv(shape)
    p = shape[2] // 2
    y = gpu_conv(x, wt, b, None, shape, 2)
    xp = torch.nn.functional.pad(x, [p] * 4, mode="reflect")
    yz = gpu_conv(xp, wt, b, None, shape[:4] + (0,) + (shape[5] + 2 * p, shape[6] + 2 * p), 2)
    assert np.abs(y).max() > 0 and np.array_equal(y.view(np.uint32), yz[p:-p, p:-p].view(np.uint32))


def test_conv_subnormal_operands():
    shape = S16.SWEEP[3]
    x, wt, b, _ = S16.draw_conv(shape, xscale=2.0 ** -6, wscale=2.0 ** -18)
    assert 0 < wt.abs().max() < 2.0 ** -14                      # every weight is an fp16 subnormal
    y = conv_case("conv subnormal %s" % (shape,), shape, 0, x, wt, b)
    assert np.abs(y).max() > 0 and np.abs(y).max() < 2.0 ** -14      # subnormal outputs, not flushed


def test_conv_rounds_fp32_operands_to_nearest_even():
    shape = S16.SWEEP[0]
    x, wt, b, _ = S16.draw_conv(shape, half=False)
    x[0, 0, 0, :4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -25])      # ties: to even, and half the smallest subnormal
    assert not is_fp16_valued(x.numpy()) and not is_fp16_valued(wt.numpy()) and not is_fp16_valued(b.numpy())
    y = gpu_conv(x, wt, b, None, shape, 3)
    yr = gpu_conv(x.half().float(), wt.half().float(), b.half().float(), None, shape, 3)
    assert np.abs(y).max() > 0 and np.array_equal(y.view(np.uint32), yr.view(np.uint32))
    assert not np.array_equal(y, gpu_conv(x, wt, b, None, shape, 3, precision="fp32"))      # and the default is another arithmetic


# ---- the nets ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amp():
    a = np.load(os.path.join(ROOT, "tests", "golden", "stage2_amp.npz"))
    return {str(n): e for n, e in zip(a["names"], a["err16"])}


@pytest.fixture(scope="module")
def nf16(g2):
    import aiod_amd
    f = aiod_amd.NeuralFilter(40, 70, precision="fp16")
    f.load_state_dicts(g2["fsd"], g2["lsd"])
    yield f
    f.close()


@pytest.fixture(scope="module")
def run16(g2, nf16):
    """The fixture clip in fp16, computed once: per frame (pred, final), and every named activation of the last frame."""
    nf16.reset()
    n = g2["pred64"].shape[0]
    frames = [tuple(a.copy() for a in nf16.frame(*_frames(g2, t))) for t in range(n)]
    import aiod_amd
    return frames, {name: nf16.activation(name) for name in aiod_amd.stage2.ACTIVATIONS}


def test_end_to_end_against_the_reference_autocast_error(g2, run16, amp):
    frames, acts = run16
    failed = []

    def check(name, hip, ref64):
        hm, hr = stats(hip, ref64)
        em, er = amp[name]
        ok = bool(np.isfinite(np.asarray(hip)).all()) and hm <= 2.0 * em and hr <= 2.0 * er
        print("%-11s hip max %.3e rms %.3e | reference autocast max %.3e rms %.3e | ratio %.2f %.2f%s" % (name, hm, hr, em, er, hm / em, hr / er, "" if ok else "  FAIL"))
        if not ok:
            failed.append(name)
    for t, (pred, final) in enumerate(frames):
        assert pred.shape == (64, 96, 3) and final.shape == (64, 96, 3)
        check("pred_%d" % t, pred, g2["pred64"][t])
        check("final_%d" % t, final, g2["final64"][t])
    torch.set_num_threads(8)
    r64 = ref_loop(g2, torch.float64, len(frames))[-1]
    assert np.abs(r64["final"] - g2["final64"][len(frames) - 1]).max() < 1e-9      # the restatement is the fixture's twin
    for name in ACTS:
        check(name, acts[name], r64[name])
    assert not failed, failed


def test_fp16_activations_are_fp16_values(run16):
    _, acts = run16
    for name, a in acts.items():
        if name == "input":               # the padded u8 / 255 frames stay fp32: the first convolutions round them as they gather
            assert not is_fp16_valued(a)
        else:
            assert np.abs(a).max() > 0 and is_fp16_valued(a), name


def test_the_mode_is_real_and_reproducible(g2, nf16, run16):
    import aiod_amd
    frames, _ = run16
    assert np.array_equal(frames[0][0], frames[0][1])               # frame 0: final == pred, bit for bit
    assert not np.array_equal(frames[1][0], frames[1][1])
    f32 = aiod_amd.NeuralFilter(40, 70)
    try:
        f32.load_state_dicts(g2["fsd"], g2["lsd"])
        for t, (pred, final) in enumerate(frames):
            p32, o32 = f32.frame(*_frames(g2, t))
            d = float(np.abs(final - o32).max())
            print("frame %d: max |fp16 - fp32| final %.3e, err32 max %.3e" % (t, d, g2["final_err32"][t][0]))
            assert d > 10.0 * g2["final_err32"][t][0] and not np.array_equal(pred, p32)
    finally:
        f32.close()
    for _ in range(2):                                              # reset reproduces, twice
        nf16.reset()
        for t, (pred, final) in enumerate(frames):
            p, o = nf16.frame(*_frames(g2, t))
            assert np.array_equal(p.view(np.uint32), pred.view(np.uint32)) and np.array_equal(o.view(np.uint32), final.view(np.uint32))


def test_switching_precision_on_one_handle(g2):
    import ctypes
    import aiod_amd
    f = aiod_amd.NeuralFilter(40, 70)
    try:
        f.load_state_dicts(g2["fsd"], g2["lsd"])
        prec = ctypes.c_int(-1)
        assert f.lib.af_filter_get_precision(f.f, ctypes.byref(prec)) == 0 and prec.value == 0 and f.precision == "fp32"
        first = [tuple(a.copy() for a in f.frame(*_frames(g2, t))) for t in range(3)]
        f.set_precision("fp16")
        assert f.lib.af_filter_get_precision(f.f, ctypes.byref(prec)) == 0 and prec.value == 1 and f.precision == "fp16"
        p, o = f.frame(*_frames(g2, 3))                             # the switch reset the recurrent state: a frame 0
        assert np.array_equal(p, o) and is_fp16_valued(p)
        with pytest.raises(aiod_amd.AtlasFitError) as e:
            f.activation("E1a")
        assert e.value.code == -5
        half = f.frame(*_frames(g2, 1))
        assert is_fp16_valued(half[1]) and not np.array_equal(half[0], half[1])
        f.set_precision("fp32")
        for t in range(3):                                          # the fp32 bits come back exactly, from a frame 0
            p, o = f.frame(*_frames(g2, t))
            assert np.array_equal(p.view(np.uint32), first[t][0].view(np.uint32)) and np.array_equal(o.view(np.uint32), first[t][1].view(np.uint32))
        assert f.lib.af_filter_set_precision(f.f, 2) == -1          # AF_EINVAL, with a message; a refused value changes nothing
        assert b"precision must be" in f.lib.af_last_error(None)
        assert f.lib.af_filter_get_precision(f.f, ctypes.byref(prec)) == 0 and prec.value == 0
        p, o = f.frame(*_frames(g2, 3))
        assert not np.array_equal(p, o)                             # ... not even the recurrent state
        with pytest.raises(ValueError):
            f.set_precision("bf16")
        x, y, w = np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 2), np.float32), np.zeros((2, 3, 1, 1), np.float32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)           # noqa: E731
        assert f.lib.af_conv2d_prec(2, 0, ptr(x), 4, 4, 3, ptr(w), None, 2, 1, 1, 0, 0, None, ptr(y), 0) == -1
        assert b"af_conv2d_prec: precision must be" in f.lib.af_last_error(None)
    finally:
        f.close()


# ---- command lines -------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_on_synthetic_tree(g2, amp, tmp_path):
    from PIL import Image
    vid, n = "clip", 3
    torch.save(g2["fsd"], tmp_path / "f.pth")
    torch.save(g2["lsd"], tmp_path / "l.pth")
    finals = {}
    for arm, extra in (("fp32", []), ("fp16", ["--filter_precision", "fp16"])):
        root = tmp_path / arm
        (root / "data" / "test" / vid).mkdir(parents=True)
        (root / "results" / vid / "stage_1" / "output").mkdir(parents=True)
        for t in range(n):
            Image.fromarray(g2["content"][t]).save(root / "data" / "test" / vid / ("%05d.png" % t))
            Image.fromarray(g2["style"][t]).resize((84, 48), Image.NEAREST).save(root / "results" / vid / "stage_1" / "output" / ("%05d.png" % t))
        _run([sys.executable, os.path.join(ROOT, "all-in-one-deflicker_amd", "neural_filter.py"), "--video_name", vid, "--ckpt_filter", str(tmp_path / "f.pth"),
              "--ckpt_local", str(tmp_path / "l.pth"), "--gpu", "0"] + extra, root)
        base = root / "results" / vid
        for d in (base / "neural_filter" / "concat", base / "neural_filter" / "output", base / "final" / "output"):
            assert sorted(os.listdir(d)) == ["%05d.png" % t for t in range(n)]
        finals[arm] = np.stack([_png(base / "final" / "output" / ("%05d.png" % t)) for t in range(n)]).astype(int)
    # two arithmetics within 2 x err16 of the fp64 twin each (fp32 far inside): 2 x max err16 in uint8 levels, + 1 for the truncation
    bound = int(np.floor(2.0 * max(amp["final_%d" % t][0] for t in range(4)) * 255)) + 1
    d = np.abs(finals["fp16"] - finals["fp32"])
    print("CLI: fp16 against fp32 final/output: %d of %d uint8 values differ, largest step %d (bound %d)" % (int((d > 0).sum()), d.size, d.max(), bound))
    assert 0 < d.max() <= bound


H, W, DOWN, SEED = 130, 197, 4, 11      # tests/test_gpu_deflicker.py's clip, config and seed
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("fp16_stage2_pipeline")
    paths = PB.write_weights(str(d / "weights"), PB.synthetic_weights())
    with open(d / "short.json", "w") as f:
        json.dump(dict(REFERENCE_CONFIG, **SHORT), f)
    return {"paths": paths, "cfg": str(d / "short.json"), "frames": PB.synthetic_clip(3, H, W, seed=5)}


def test_in_process_route_equals_the_chained_clis(clip, tmp_path):
    import pipeline_bench as PB
    n = len(clip["frames"])
    roots = {arm: tmp_path / arm for arm in ("in_process", "chained")}
    for r in roots.values():
        PB.write_clip(str(r / "data" / "test" / "clip"), clip["frames"])
    out = roots["in_process"] / "out"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(out), clip["cfg"], DOWN, SEED, clip["paths"],
                               extra=["--keep_intermediates", "--filter_precision", "fp16"]), tmp_path)
    for name, cmd in PB.chained_commands("clip", clip["cfg"], DOWN, SEED, clip["paths"]):
        _run(cmd + (["--filter_precision", "fp16"] if name == "stage 2" else []), roots["chained"])
    assert json.load(open(out / "deflicker.json"))["filter_precision"] == "fp16"
    ref = roots["chained"] / "results" / "clip"
    names = ["%05d.png" % i for i in range(n)]
    for sub in (("neural_filter", "output"), ("neural_filter", "concat"), ("final", "output")):
        a, b = out.joinpath(*sub), ref.joinpath(*sub)
        assert sorted(os.listdir(a)) == names == sorted(os.listdir(b)), sub
        for fn in names:
            x, y = _png(a / fn), _png(b / fn)
            assert x.shape == y.shape and np.array_equal(x, y), "%s/%s differs in %d values" % ("/".join(sub), fn, int((x != y).sum()))
    # without the flag: the record says fp32, and the frames are other frames
    plain = tmp_path / "plain"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(plain), clip["cfg"], DOWN, SEED, clip["paths"]), tmp_path)
    assert json.load(open(plain / "deflicker.json"))["filter_precision"] == "fp32"
    assert any(not np.array_equal(_png(plain / "final" / "output" / fn), _png(out / "final" / "output" / fn)) for fn in names)
