"""sha256 digests of everything the implicit-GEMM convolution core (csrc/conv_gemm.h: k_conv of stage 2, k_rconv of RAFT) feeds, to
compare two builds of the library bit for bit (MEASUREMENTS.md Part L).  Only the public Python API is used, so the same file runs
on an older tree: copy it, and tests/test_gpu_raft.py for its case list, into that tree and run it there.  The inputs of the stand-alone
cases are drawn as test_conv2d_sweep, test_rect_conv and test_gru_half draw theirs; a change of those tests' inputs belongs here too.

    python tools/conv_paths_digest.py OUT.json              # write {"count": N, "digests": {name: sha256}}
    python tools/conv_paths_digest.py OUT.json --compare OTHER.json      # ... and exit 1 unless every digest equals OTHER's

Digested, all fp32 as the library returns them:
  stage 2   pred, final and every named activation of the 4 frames of tests/golden/stage2.npz (the refinement net's on frames 1-3);
            every output of CONV_CASES of tests/test_gpu_stage2.py, on that test's inputs
  RAFT      the tests/golden/raft.npz pair at capacity 2: both saved flows and both 1/8 flows after 20 iterations, every named
            activation (corr_vol0..3 included) after iteration 1, the five test_rect_conv cases and both gru_half directions of
            tests/test_gpu_raft.py, on those tests' inputs"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def shapes(table):
    return [tuple(int(v) for v in r if v >= 0) for r in table]


def stage2(out):
    import aiod_amd
    import test_gpu_stage2 as T
    from make_golden_stage2 import synthetic_state_dicts
    g2 = dict(np.load(T.GOLDEN))
    fsd = {str(k): torch.zeros(s) for k, s in zip(g2["filter_keys"], shapes(g2["filter_shapes"]))}      # the weights of the test's fixture
    lsd = {str(k): torch.zeros(s) for k, s in zip(g2["local_keys"], shapes(g2["local_shapes"]))}
    for k in lsd:
        if k.endswith("num_batches_tracked"):
            lsd[k] = torch.zeros((), dtype=torch.int64)
    synthetic_state_dicts(fsd, lsd)
    nf = aiod_amd.NeuralFilter(40, 70)
    nf.load_state_dicts(fsd, lsd)
    for t in range(g2["content"].shape[0]):
        pred, final = nf.frame(g2["content"][t] / 255.0, g2["style"][t] / 255.0)
        out["stage2/frame%d/pred_out" % t], out["stage2/frame%d/final_out" % t] = sha(pred), sha(final)
        for name in aiod_amd.stage2.ACTIVATIONS:
            try:
                out["stage2/frame%d/%s" % (t, name)] = sha(nf.activation(name))
            except aiod_amd.AtlasFitError:      # frame 0: the refinement net did not run
                assert t == 0, (t, name)
    nf.close()
    g = torch.Generator().manual_seed(7)        # the inputs of test_conv2d_sweep, drawn in its order
    for i, (cin, cout, k, stride, pm, act, has_b, has_r, h, w) in enumerate(T.CONV_CASES):
        x = torch.rand(h, w, cin, generator=g, dtype=torch.float64) * 2 - 1
        wt = (torch.rand(cout, cin, k, k, generator=g, dtype=torch.float64) * 2 - 1) * np.sqrt(6.0 / (cin * k * k))
        b = (torch.rand(cout, generator=g, dtype=torch.float64) - 0.5) * 0.1 if has_b else None
        r = torch.rand((h - 1) // stride + 1, (w - 1) // stride + 1, cout, generator=g, dtype=torch.float64) if has_r else None
        a = [None if v is None else v.float().numpy() for v in (x, wt, b, r)]
        out["stage2/conv_case%02d" % i] = sha(aiod_amd.stage2.conv2d(a[0], a[1], a[2], stride, pm, act, a[3]))


def raft(out):
    import aiod_amd
    import test_gpu_raft as T
    from aiod_amd.raft import conv2d, gru_half
    g = dict(np.load(T.GOLDEN))
    sd = {str(k): torch.zeros(s, dtype=torch.int64 if str(k).endswith("num_batches_tracked") else torch.float32)
          for k, s in zip(g["keys"], shapes(g["shapes"]))}                                                    # the weights of the test's fixture
    T.G.synthetic_state_dict(sd)
    r = aiod_amd.RAFT(T.H, T.W, capacity=2)
    r.load_state_dict(sd)
    r.encode(0, g["im1"])
    r.encode(1, g["im2"])
    up, lo = r.flow_slots([(0, 1), (1, 0)], iters=20, want_lo=True)
    for i, d in enumerate(("12", "21")):
        out["raft/up" + d], out["raft/lo%s_20" % d] = sha(up[i]), sha(lo[i])
    r.flow_slots([(0, 1)], iters=1)
    for name in list(aiod_amd.raft.ACTIVATIONS) + ["corr_vol%d" % l for l in range(4)]:
        out["raft/iter1/" + name] = sha(r.activation(name))
    r.close()
    for kh, kw, cin, cout, act in T.RECT_CASES:
        gen = torch.Generator().manual_seed(100 * kh + kw + cin)
        x = torch.randn((2, cin, 19, 27), generator=gen)
        wt = (torch.rand((cout, cin, kh, kw), generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (cin * kh * kw)))
        b = (torch.rand((cout,), generator=gen) * 2 - 1) * 0.05
        out["raft/rect_conv_%dx%d_%d_%d_act%d" % (kh, kw, cin, cout, act)] = sha(conv2d(x.permute(0, 2, 3, 1).numpy(), wt.numpy(), b.numpy(), act=act))
    for vertical in (0, 1):
        gen = torch.Generator().manual_seed(7 + vertical)
        k = (5, 1) if vertical else (1, 5)
        net = torch.tanh(torch.randn((2, 128, 17, 25), generator=gen))
        x = torch.randn((2, 256, 17, 25), generator=gen)
        ws = [(torch.rand((128, 384) + k, generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (384 * 5))) for _ in range(3)]
        bs = [(torch.rand((128,), generator=gen) * 2 - 1) * 0.05 for _ in range(3)]
        out["raft/gru_half_vertical%d" % vertical] = sha(gru_half(net.permute(0, 2, 3, 1).numpy(), x.permute(0, 2, 3, 1).numpy(), ws[0].numpy(), bs[0].numpy(),
                                                                   ws[1].numpy(), bs[1].numpy(), ws[2].numpy(), bs[2].numpy(), vertical))


def main():
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4 and sys.argv[2] != "--compare"):
        sys.exit(__doc__)
    out = {}
    stage2(out)
    raft(out)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump({"count": len(out), "digests": out}, f, indent=1, sort_keys=True)
    print("%d digests -> %s" % (len(out), sys.argv[1]))
    if len(sys.argv) == 4:
        with open(sys.argv[3]) as f:
            other = json.load(f)["digests"]
        bad = sorted(k for k in set(out) | set(other) if out.get(k) != other.get(k))
        print("compared with %s: %d of %d differ%s" % (sys.argv[3], len(bad), len(set(out) | set(other)), "".join("\n  " + k for k in bad)))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
