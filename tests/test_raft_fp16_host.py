"""Host-side checks of the native RAFT path's precision mode "fp16" (no GPU): the rounding contract itself, pinned on the CPU against
the reference's own fp16-autocast error (tests/golden/raft_amp.npz, tools/make_golden_raft_amp.py), and the flag's way through the
command builders and the one-process pipeline.

Rule (the project's usual one): max and rms of |contract twin - fp64 twin| are each at most twice the same statistic of |reference
under fp16 autocast - fp64 twin| recorded in raft_amp.npz.  The contract twin is tests/raft_fp16_ref.py, in fp64 and in fp32."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_raft as G  # noqa: E402
import raft_fp16_ref as R16  # noqa: E402

INTERMEDIATES = ("fmap1", "fmap2", "net0", "inp", "motion", "net", "delta", "mask")


def _stats(a, ref64):
    d = np.abs(np.asarray(a, np.float64) - ref64).ravel()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


def _hwc(t):
    return t[0].permute(1, 2, 0).double().numpy()


@pytest.fixture(scope="module")
def g():
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "raft.npz")))
    amp = np.load(os.path.join(ROOT, "tests", "golden", "raft_amp.npz"))
    for k in ("up12", "up21"):
        d[k] = d[k + "_hi"].astype(np.float64) + d[k + "_lo"].astype(np.float64) / G.LO_SCALE
    sd = {}
    for k, r in zip(d["keys"], d["shapes"]):
        shape = tuple(int(v) for v in r if v >= 0)
        sd[str(k)] = torch.zeros(shape, dtype=torch.int64 if str(k).endswith("num_batches_tracked") else torch.float32)
    G.synthetic_state_dict(sd)
    d["sd"] = {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}
    d["im"] = [G.pad_sintel(G.to_nchw(d["im1"])), G.pad_sintel(G.to_nchw(d["im2"]))]
    d["amp_names"] = [str(n) for n in amp["names"]]
    d["err16"] = {str(n): e for n, e in zip(amp["names"], amp["err16"])}
    torch.set_num_threads(8)
    d["acts64"] = {}
    G.raft_forward(d["sd"][torch.float64], d["im"][0].double(), d["im"][1].double(), iters=1, acts=d["acts64"])
    return d


def test_fixture_lists_exactly_the_fp32_fixtures_names(g):
    assert g["amp_names"] == [str(n) for n in g["names"]]
    assert all(np.isfinite(e).all() and (e > 0).all() for e in g["err16"].values())
    # the autocast rebinding took: the reference's fp16 error is far above its fp32 error
    err32 = {str(n): e for n, e in zip(g["names"], g["err32"])}
    assert g["err16"]["up12"][0] > 100 * err32["up12"][0]


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_contract_sits_at_the_reference_autocast_error(g, dt):
    sd = g["sd"][dt]
    bad = []

    def check(name, v, ref64):
        m, r = _stats(v, ref64)
        em, er = g["err16"][name]
        print("%-8s contract %s max %.3e rms %.3e | reference autocast max %.3e rms %.3e | ratio %.2f %.2f" % (name, dt, m, r, em, er, m / em, r / er))
        if not (np.isfinite(m) and m <= 2 * em and r <= 2 * er):
            bad.append(name)
    acts = {}
    R16.raft_forward(sd, g["im"][0].to(dt), g["im"][1].to(dt), iters=1, acts=acts)
    for n in INTERMEDIATES:
        check(n, _hwc(acts[n]), _hwc(g["acts64"][n]))
    for d, (a, b) in (("12", (0, 1)), ("21", (1, 0))):
        _, up = R16.raft_forward(sd, g["im"][a].to(dt), g["im"][b].to(dt), iters=20)
        check("up" + d, _hwc(up), g["up" + d])
    assert not bad, bad


def test_rounding_points_produce_fp16_values(g):
    acts = {}
    R16.raft_forward(g["sd"][torch.float32], g["im"][0], g["im"][1], iters=3, acts=acts)      # the flow is zero in iteration 1 and one fp16 delta in iteration 2
    for n in ("fmap1", "net0", "inp", "net", "delta", "mask"):
        assert torch.equal(R16.q(acts[n]), acts[n]), n
    assert torch.equal(R16.q(acts["motion"][:, :126]), acts["motion"][:, :126])
    assert not torch.equal(R16.q(acts["motion"][:, 126:]), acts["motion"][:, 126:])      # the flow channels stay fp32


# ---- flag plumbing ---------------------------------------------------------------------------------------------------------
def _stage1_args(argv, two_layer=False):
    from aiod_amd import stage1
    a = stage1._parse_args(argv, two_layer)
    a.device_ordinal, a.vid_path = 0, os.path.join(a.root, a.vid_name)
    return a


@pytest.mark.parametrize("two_layer", [False, True])
def test_stage1_command_builder_passes_the_flag_on(two_layer):
    from aiod_amd import stage1
    base = ["--vid_name", "clip"]
    plain = stage1._preprocessor_commands(_stage1_args(base + ["--native_flow"], two_layer), two_layer)
    fp32 = stage1._preprocessor_commands(_stage1_args(base + ["--native_flow", "--flow_precision", "fp32"], two_layer), two_layer)
    fp16 = stage1._preprocessor_commands(_stage1_args(base + ["--native_flow", "--flow_precision", "fp16"], two_layer), two_layer)
    assert plain == fp32 and "flow_precision" not in plain[0]           # the default command is the command as it was
    assert fp16[0] == plain[0] + "--flow_precision fp16 " and fp16[1:] == plain[1:]
    assert "preprocess_optical_flow.py" in fp16[0]
    without = stage1._preprocessor_commands(_stage1_args(base, two_layer), two_layer)
    assert all("flow_precision" not in c for c in without)


@pytest.mark.parametrize("two_layer", [False, True])
def test_stage1_flag_needs_native_flow(two_layer, capsys):
    from aiod_amd import stage1
    with pytest.raises(SystemExit) as e:
        stage1._parse_args(["--vid_name", "clip", "--flow_precision", "fp16"], two_layer)
    assert e.value.code == 2 and "--native_flow" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        stage1._parse_args(["--vid_name", "clip", "--native_flow", "--flow_precision", "bf16"], two_layer)
    assert stage1._parse_args(["--vid_name", "clip"], two_layer).flow_precision == "fp32"


def test_run_pipeline_forwards_the_flag(capsys):
    from aiod_amd import run_pipeline as RP
    base = ["--video_frame_folder", "data/test/clip"]
    plain = RP.build_commands(RP.parse_opts(base + ["--native_flow"]))
    fp16 = RP.build_commands(RP.parse_opts(base + ["--native_flow", "--flow_precision", "fp16"]))
    stage1_plain = [c for _, c in plain if "stage1.py" in c]
    stage1_fp16 = [c for _, c in fp16 if "stage1.py" in c]
    assert len(stage1_plain) == 1 and "flow_precision" not in stage1_plain[0]
    assert stage1_fp16 == [stage1_plain[0].replace(" --native_flow", " --native_flow --flow_precision fp16")]
    assert [c for c in fp16 if "stage1.py" not in c[1]] == [c for c in plain if "stage1.py" not in c[1]]
    seg = RP.build_commands(RP.parse_opts(base + ["--native_flow", "--flow_precision", "fp16", "--class_name", "portrait"]))
    assert any("stage1_seg.py" in c and c.endswith("--native_flow --flow_precision fp16") for _, c in seg)
    one = RP.build_commands(RP.parse_opts(base + ["--in_process", "--flow_precision", "fp16"]))
    assert one[-1][1].endswith(" --flow_precision fp16") and "deflicker.py" in one[-1][1]
    with pytest.raises(SystemExit) as e:
        RP.parse_opts(base + ["--flow_precision", "fp16"])
    assert e.value.code == 2 and "--native_flow" in capsys.readouterr().err


def test_precompute_cli_flag():
    from aiod_amd import preprocess_optical_flow as POF
    assert POF.parse_args([]).flow_precision == "fp32"
    assert POF.parse_args(["--flow_precision", "fp16"]).flow_precision == "fp16"
    with pytest.raises(SystemExit):
        POF.parse_args(["--flow_precision", "half"])


def test_bad_precision_names_raise_before_any_work():
    import aiod_amd
    from aiod_amd import raft
    x = np.zeros((1, 4, 4, 3), np.float32)
    for call in (lambda: aiod_amd.RAFT(130, 197, precision="half"),
                 lambda: raft.conv2d(x, np.zeros((2, 3, 1, 1), np.float32), precision="bf16"),
                 lambda: raft.instance_norm(np.zeros((4, 4, 64), np.float32), precision=16),
                 lambda: raft.gru_half(None, None, None, None, None, None, None, None, 0, precision="FP16")):
        with pytest.raises(ValueError, match="fp32, fp16"):
            call()
    with pytest.raises(ValueError, match="flow_precision must be one of fp32, fp16"):
        aiod_amd.Deflicker(None, None, None, flow_precision="half", engines=object())
    assert raft.precision_code("fp32") == 0 and raft.precision_code("fp16") == 1


def test_deflicker_hands_the_precision_to_open_flow_and_records_it():
    import aiod_amd
    import test_deflicker_host as DH

    class Engines(DH._StubEngines):
        def open_flow(self, h, w, **kw):
            self.log.append(("raft_open", h, w) + tuple(sorted(kw.items())))
            return DH._StubFlow(self.log, h, w)

    logs = {}
    for name, kw in (("default", {}), ("fp32", {"flow_precision": "fp32"}), ("fp16", {"flow_precision": "fp16"})):
        E = Engines()
        d = aiod_amd.Deflicker(None, None, None, config=DH.SMALL, down=4, seed=7, engines=E, **kw)
        res = d.run(DH._frames(4), keep=("final",))
        assert res["flow_precision"] == ("fp16" if name == "fp16" else "fp32")
        logs[name] = E.log
    assert [e for e in logs["default"] if e[0] == "raft_open"] == [("raft_open", 8, 12)]      # the call as it was: no new argument
    assert logs["fp32"] == logs["default"]
    assert [e for e in logs["fp16"] if e[0] == "raft_open"] == [("raft_open", 8, 12, ("precision", "fp16"))]
    assert [e for e in logs["fp16"] if e[0] != "raft_open"] == [e for e in logs["default"] if e[0] != "raft_open"]
    # the unchanged stub of tests/test_deflicker_host.py (open_flow(h, w)) still serves the default
    E = DH._StubEngines()
    aiod_amd.Deflicker(None, None, None, config=DH.SMALL, down=4, seed=7, engines=E).run(DH._frames(4), keep=("final",))
    assert E.log == logs["default"]


def test_deflicker_cli_flag():
    from aiod_amd import deflicker
    assert deflicker.parse_args(["--frames_dir", "x"]).flow_precision == "fp32"
    assert deflicker.parse_args(["--frames_dir", "x", "--flow_precision", "fp16"]).flow_precision == "fp16"
    with pytest.raises(SystemExit):
        deflicker.parse_args(["--frames_dir", "x", "--flow_precision", "fp8"])
