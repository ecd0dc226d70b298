"""Host-side checks of stage 2's precision mode "fp16" (no GPU): the rounding contract itself, pinned on the CPU against the
reference's own fp16-autocast error (tests/golden/stage2_amp.npz, tools/make_golden_stage2_amp.py), the claim that an
fp32-accumulating implementation can meet the GPU sweep's 1 % cap, and the flag's way through the command lines and the pipeline.

Rule (the project's usual one): max and rms of |contract twin - fp64 twin| are each at most twice the same statistic of |reference
under fp16 autocast - fp64 twin| recorded in stage2_amp.npz.  The contract twin is tests/stage2_fp16_ref.py, in fp64 and in fp32."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_stage2 as G  # noqa: E402
import stage2_fp16_ref as S16  # noqa: E402
from test_gpu_stage2 import ref_loop, _shapes  # noqa: E402

ACTS = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec4", "dec3", "dec2", "dec1", "E3", "RB")


def _stats(a, ref64):
    d = np.abs(np.asarray(a, np.float64) - ref64).ravel()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


@pytest.fixture(scope="module")
def g2():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "stage2.npz")))
    amp = np.load(os.path.join(ROOT, "tests", "golden", "stage2_amp.npz"))
    for w in ("pred", "final"):
        g[w + "64"] = g[w + "64_hi"].astype(np.float64) + g[w + "64_lo"].astype(np.float64) / G.LO_SCALE
    fsd = {str(k): torch.zeros(s) for k, s in zip(g["filter_keys"], _shapes(g["filter_shapes"]))}
    lsd = {str(k): torch.zeros(s) for k, s in zip(g["local_keys"], _shapes(g["local_shapes"]))}
    G.synthetic_state_dicts(fsd, lsd)
    g["fsd"], g["lsd"] = fsd, {k: v for k, v in lsd.items() if "norm_layer" not in k}
    g["amp_names"] = [str(n) for n in amp["names"]]
    g["err16"] = {str(n): e for n, e in zip(amp["names"], amp["err16"])}
    torch.set_num_threads(8)
    g["acts64"] = ref_loop(g, torch.float64, G.NF)[-1]
    g["cs"] = [G.pad_other(t) for t in G.to_nchw(g["content"])]
    g["ss"] = [G.pad_other(t) for t in G.to_nchw(g["style"])]
    return g


def test_fixture_names_and_level(g2):
    assert g2["amp_names"] == ["%s_%d" % (w, t) for t in range(G.NF) for w in ("pred", "final")] + list(ACTS)
    assert all(np.isfinite(e).all() and (e > 0).all() for e in g2["err16"].values())
    # the autocast took: the reference's fp16 error is far above its fp32 error, and below one uint8 level
    assert g2["err16"]["pred_3"][0] > 100 * g2["pred_err32"][3][0]
    assert max(g2["err16"]["final_%d" % t][0] for t in range(G.NF)) < 1.0 / 255


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_contract_sits_at_the_reference_autocast_error(g2, dt):
    out = S16.loop(g2["fsd"], g2["lsd"], g2["cs"], g2["ss"], dt)
    bad = []

    def check(name, v, ref64):
        m, r = _stats(v, ref64)
        em, er = g2["err16"][name]
        print("%-11s contract %s max %.3e rms %.3e | reference autocast max %.3e rms %.3e | ratio %.2f %.2f" % (name, dt, m, r, em, er, m / em, r / er))
        if not (np.isfinite(m) and m <= 2 * em and r <= 2 * er):
            bad.append(name)
    for t in range(G.NF):
        for w in ("pred", "final"):
            check("%s_%d" % (w, t), out[t][w], g2[w + "64"][t])
    for n in ACTS:
        check(n, out[-1][n], g2["acts64"][n])
    assert not bad, bad
    assert np.array_equal(out[0]["pred"], out[0]["final"])                        # frame 0
    for n, v in out[-1].items():                                                   # every rounding point holds fp16 values
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v) == (n != "input"), n


@pytest.mark.parametrize("shape", S16.SWEEP, ids=lambda s: "x".join(str(v) for v in s))
def test_fp32_accumulation_meets_the_one_percent_cap(shape):
    """What a correct kernel can reach: the restatement with fp32 sums, and torch's own half convolution, against the fp64 twin."""
    worst = 0.0
    for act in range(4):
        x, wt, b, _ = S16.draw_conv(shape)
        twin = S16.conv2d(x.double(), wt.double(), b.double(), shape[3], shape[4], act)
        r32 = S16.conv2d(x, wt, b, shape[3], shape[4], act).double()
        th = S16.torch_half_conv(x, wt, b, shape[3], shape[4], act)
        f32, fh = float((r32 != twin).double().mean()), float((th != twin).double().mean())
        print("%s act %d: fp32 restatement differs on %.3f %%, torch half on %.3f %%" % (shape, act, 100 * f32, 100 * fh))
        worst = max(worst, f32)
    assert worst <= 0.01


# ---- flags and stubs -----------------------------------------------------------------------------------------------------------
def test_bad_precision_names_raise_before_any_work():
    import aiod_amd
    from aiod_amd import stage2
    for call in (lambda: aiod_amd.NeuralFilter(40, 70, precision="half"),
                 lambda: stage2.conv2d(np.zeros((4, 4, 3), np.float32), np.zeros((2, 3, 1, 1), np.float32), precision="bf16")):
        with pytest.raises(ValueError, match="fp32, fp16"):
            call()
    with pytest.raises(ValueError, match="filter_precision must be one of fp32, fp16"):
        aiod_amd.Deflicker(None, None, None, filter_precision="bf16", engines=object())
    assert stage2.precision_code("fp32") == 0 and stage2.precision_code("fp16") == 1


def test_cli_flags(capsys):
    from aiod_amd import deflicker, neural_filter
    from aiod_amd import run_pipeline as RP
    assert neural_filter.parse_args([]).filter_precision == "fp32"
    assert neural_filter.parse_args(["--filter_precision", "fp16"]).filter_precision == "fp16"
    assert deflicker.parse_args(["--frames_dir", "x"]).filter_precision == "fp32"
    assert deflicker.parse_args(["--frames_dir", "x", "--filter_precision", "fp16"]).filter_precision == "fp16"
    for mod, base in ((neural_filter, []), (deflicker, ["--frames_dir", "x"])):
        with pytest.raises(SystemExit):
            mod.parse_args(base + ["--filter_precision", "bf16"])
    base = ["--video_frame_folder", "data/test/clip"]
    plain = RP.build_commands(RP.parse_opts(base + ["--native_stage2"]))
    fp32 = RP.build_commands(RP.parse_opts(base + ["--native_stage2", "--filter_precision", "fp32"]))
    fp16 = RP.build_commands(RP.parse_opts(base + ["--native_stage2", "--filter_precision", "fp16"]))
    assert plain == fp32 and all("filter_precision" not in c for _, c in plain)      # the default commands are the commands as they were
    assert fp16[:-1] == plain[:-1] and fp16[-1] == (plain[-1][0], plain[-1][1] + " --filter_precision fp16") and "neural_filter.py" in fp16[-1][1]
    one = RP.build_commands(RP.parse_opts(base + ["--in_process", "--filter_precision", "fp16"]))
    assert one[-1][1].endswith(" --filter_precision fp16") and "deflicker.py" in one[-1][1]
    with pytest.raises(SystemExit) as e:
        RP.parse_opts(base + ["--filter_precision", "fp16"])
    assert e.value.code == 2 and "--native_stage2" in capsys.readouterr().err


def test_deflicker_hands_the_precision_to_open_filter_and_records_it():
    import aiod_amd
    import test_deflicker_host as DH

    class Engines(DH._StubEngines):
        def open_filter(self, h, w, **kw):
            self.log.append(("filter_open", h, w) + tuple(sorted(kw.items())))
            return DH._StubFilter(self.log)

    logs = {}
    for name, kw in (("default", {}), ("fp32", {"filter_precision": "fp32"}), ("fp16", {"filter_precision": "fp16"})):
        E = Engines()
        res = aiod_amd.Deflicker(None, None, None, config=DH.SMALL, down=4, seed=7, engines=E, **kw).run(DH._frames(4), keep=("final",))
        assert res["filter_precision"] == ("fp16" if name == "fp16" else "fp32") and res["flow_precision"] == "fp32"
        logs[name] = E.log
    assert [e for e in logs["default"] if e[0] == "filter_open"] == [("filter_open", 8, 12)]      # the call as it was: no new argument
    assert logs["fp32"] == logs["default"]
    assert [e for e in logs["fp16"] if e[0] == "filter_open"] == [("filter_open", 8, 12, ("precision", "fp16"))]
    assert [e for e in logs["fp16"] if e[0] != "filter_open"] == [e for e in logs["default"] if e[0] != "filter_open"]
    # the unchanged stub of tests/test_deflicker_host.py (open_filter(h, w)) still serves the default
    E = DH._StubEngines()
    aiod_amd.Deflicker(None, None, None, config=DH.SMALL, down=4, seed=7, engines=E).run(DH._frames(4), keep=("final",))
    assert E.log == logs["default"]
