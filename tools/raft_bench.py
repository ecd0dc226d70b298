"""Time of the flow precompute on one MI355X: the native RAFT forward (aiod_amd.RAFT) in fp32 (`native_cap<n>`) and in its fp16
precision mode (`native_fp16_cap<n>`: the arithmetic the reference uses on a GPU) against the pure-torch restatement of
tools/make_golden_raft.py on PyTorch-ROCm in fp32 and under fp16 autocast, in one process, alternating the arms.  The two fp16 arms
are a DIFFERENT, less accurate arithmetic than the two fp32 arms: compare within a pair.

    python tools/raft_bench.py [--sizes 768x432,1920x1080] [--rounds 5] [--capacity 2] [--frames 80] [--out raft_bench.json]

Per size: synthetic weights (the fixture's fill) and two smooth frames.  Both arms work on device-resident data: the native arm takes
its frames as CUDA tensors and writes its flows into CUDA tensors (on_device), the torch arm keeps everything on the device; no arm
copies to or from the host inside a timed span.  Every shape is run once untimed first.  A sample is the host clock around one call
between two device synchronisations (the native handle runs on its own stream and its calls return synchronised, so events on torch's
stream would not bracket it; the host clock brackets both arms the same way; one call is 20-2000 ms, far above the clock's and the
launch path's noise).  Medians over the rounds with min / max.  Reported per arm:
  encode_ms   one frame through fnet + cnet (native) / fnet on both frames + cnet as the reference's forward does it (torch)
  dir_ms      one pair-direction: correlation + 20 iterations + upsampling (native: a batch of `capacity` directions / capacity;
              torch: the whole forward, encoders included, as the reference has no frame cache)
  clip_s      an F-frame clip, 2 (F - 1) directions: native F * encode + 2 (F - 1) * dir; torch 2 (F - 1) * dir
The native arms are also run at capacity 1 to show what running both directions of a pair in one launch buys."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_raft as G  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": v[0], "max": v[-1], "n": len(v)}


def frames(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def f(dx, dy):
        x, y = xx - dx, yy - dy
        ch = [0.5 + 0.25 * np.sin(2 * np.pi * (x / 37.0 * (1 + 0.3 * c) + y / 53.0) + c) + 0.2 * np.cos(2 * np.pi * (y / 29.0 - x / 71.0 * (1 + c))) for c in range(3)]
        return np.round(np.clip(np.stack(ch, -1), 0, 1) * 255).astype(np.float32)
    return f(0, 0), f(3, -2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x432,1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=2)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_torch", action="store_true")
    args = ap.parse_args()
    import aiod_amd
    from aiod_amd.raft import raft_keys
    sd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in raft_keys()}
    G.synthetic_state_dict(sd)
    dev = torch.device("cuda:0")
    sdg = {k: v.to(dev) for k, v in sd.items()}
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "frames": args.frames, "sizes": {}}
    F_ = args.frames
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        u1, u2 = frames(h, w)
        t1, t2 = (G.pad_sintel(torch.from_numpy(u).permute(2, 0, 1)[None]).to(dev) for u in (u1, u2))
        d1, d2 = torch.from_numpy(u1).to(dev), torch.from_numpy(u2).to(dev)
        arms = {}
        nat = {}
        for prec, tag in (("fp32", "native"), ("fp16", "native_fp16")):
            for cap in sorted({1, args.capacity}):
                r = aiod_amd.RAFT(h, w, capacity=cap, precision=prec)
                r.load_state_dict(sd)
                pairs = [(0, 1), (1, 0), (0, 1), (1, 0)][:cap] if cap <= 4 else [(i & 1, 1 - (i & 1)) for i in range(cap)]
                nat["%s_cap%d" % (tag, cap)] = (r, pairs, cap)
                r.encode(0, d1); r.encode(1, d2); r.flow_slots(pairs, args.iters, on_device=True)      # warm-up of every shape
                arms["%s_cap%d" % (tag, cap)] = {"encode": [], "flow": []}
        torch_arms = [] if args.skip_torch else [("torch_fp32", False), ("torch_fp16_autocast", True)]
        for name, amp in torch_arms:
            G.raft_forward(sdg, t1, t2, iters=args.iters, amp=amp)                         # warm-up
            arms[name] = {"dir": []}
        for _ in range(args.rounds):                                                       # alternate the arms inside every round
            for name, (r, pairs, cap) in nat.items():
                a = arms[name]
                a["encode"].append(timed(lambda: r.encode(0, d1)))
                a["flow"].append(timed(lambda: r.flow_slots(pairs, args.iters, on_device=True)))
            for name, amp in torch_arms:
                arms[name]["dir"].append(timed(lambda: G.raft_forward(sdg, t1, t2, iters=args.iters, amp=amp)))
        out = {}
        for name, (r, pairs, cap) in nat.items():
            a = arms[name]
            enc, flow = summary(a["encode"]), summary(a["flow"])
            d = flow["median"] / cap
            out[name] = {"encode_ms": enc, "batch_ms": flow, "dir_ms": d, "clip_s": (F_ * enc["median"] + 2 * (F_ - 1) * d) / 1e3}
            r.close()
        for name, _ in torch_arms:
            s = summary(arms[name]["dir"])
            out[name] = {"dir_ms": s, "clip_s": 2 * (F_ - 1) * s["median"] / 1e3}
        res["sizes"][size] = out
        print(size, json.dumps(out), flush=True)
        del nat
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
