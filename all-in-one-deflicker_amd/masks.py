"""Keyframe masks: fg masks painted on a few frames of a clip, carried to every other frame along the optical flows.

The fg/bg two-layer path wants one mask per frame.  The reference gets them from external segmentation models this package does not
run; the masks only bootstrap the alpha net (alpha_bootstrapping_loss until stop_bootstrapping_iteration), so coarse ones are enough.
Here a user paints two or three key masks and the rest are propagated on the device, at the stage-1 size, with the flows the pipeline
has already computed.

One step (af_mask_step, csrc/maskprop.hip) carries a mask m and a confidence c from a frame s to a neighbour t: a target pixel looks
its source up along the flow t -> s, bilinearly, where the look-up lands in the frame and the round trip through the flow s -> t
closes within `thresh` pixels (the reference's flow filter, unwrap_utils.py:10-23); elsewhere (disoccluded, out of frame) the target
keeps the source's value at its own position with confidence 0.  A key has confidence 1.  A frame between two keys a < t < b gets a
forward chain from a, a backward chain from b and their blend (af_mask_blend), weighted by confidence and by the distance to the
other key; a frame outside the keys of its shot gets the one chain that reaches it.  Propagation never crosses a scene cut.

`thresh` and the hold rule are policy: nobody has measured propagated masks as mattes on footage."""
import numpy as np

from ._residence import Host, one_device

DEFAULT_THRESH = 1.0


def plan_mask_propagation(n, keys, shots=None):
    """The steps that give every frame of an n-frame clip a mask from the key frames `keys`, per shot: a list with one entry per shot
    of `shots` ([(start, stop)], default one shot), each the ordered list of that shot's steps
        ("key", t)              frame t is a key: its mask as given, confidence 1
        ("step", s, t)          one af_mask_step from frame s to its neighbour t = s +- 1, continuing the chain that reached s in
                                that direction (t > s: the forward chain, t < s: the backward chain; a key starts both)
        ("blend", a, t, b)      frame t between the keys a < t < b: af_mask_blend of the forward and the backward chain at t.
    Frames before a shot's first key hang on one backward chain, frames after its last key on one forward chain; an interval between two
    keys is walked once in each direction, not once per frame.  ValueError for no keys, a key outside 0..n-1 and a shot without a key."""
    n = int(n)
    keys = sorted(set(int(k) for k in keys))
    if not keys:
        raise ValueError("plan_mask_propagation: no key masks (at least one frame of every shot needs one)")
    for k in keys:
        if k < 0 or k >= n:
            raise ValueError("plan_mask_propagation: key %d is outside 0..%d (the clip has %d frames)" % (k, n - 1, n))
    plans = []
    for i, (lo, hi) in enumerate([(0, n)] if shots is None else list(shots)):
        lo, hi = int(lo), int(hi)
        own = [k for k in keys if lo <= k < hi]
        if not own:
            raise ValueError("plan_mask_propagation: shot %d (frames %d..%d) holds no key mask: propagation does not cross a cut" % (i, lo, hi - 1))
        steps = [("key", k) for k in own]
        steps += [("step", s, s - 1) for s in range(own[0], lo, -1)]
        for a, b in zip(own[:-1], own[1:]):
            steps += [("step", s, s + 1) for s in range(a, b - 1)]
            steps += [("step", s, s - 1) for s in range(b, a + 1, -1)]
            steps += [("blend", a, t, b) for t in range(a + 1, b)]
        steps += [("step", s, s + 1) for s in range(own[-1], hi - 1)]
        plans.append(steps)
    return plans


def _check_thresh(thresh):
    t = float(thresh)
    if not np.isfinite(t) or t <= 0:
        raise ValueError("mask propagation: thresh must be finite and > 0, got %r" % (thresh,))
    return t


def _shots_of(flows12, flows21, shots):
    """The shots propagation runs in: as given, else the runs of pairs that have flows (a pair without one is a cut)."""
    n = len(flows12) + 1
    if len(flows21) != len(flows12):
        raise ValueError("mask propagation: %d forward and %d backward flows" % (len(flows12), len(flows21)))
    for i, (a, b) in enumerate(zip(flows12, flows21)):
        if (a is None) != (b is None):
            raise ValueError("mask propagation: pair %d has a flow in one direction only" % i)
    if shots is None:
        starts = [0] + [i + 1 for i, f in enumerate(flows12) if f is None]
        return [(a, b) for a, b in zip(starts, starts[1:] + [n])]
    for a, b in shots:
        for i in range(int(a), int(b) - 1):
            if flows12[i] is None:
                raise ValueError("mask propagation: pair %d inside shot %d..%d has no flow" % (i, a, b - 1))
    return [(int(a), int(b)) for a, b in shots]


def _propagate(keys, flows12, flows21, shots, step, blend, ones):
    """Runs plan_mask_propagation's steps.  step(m, c, f_ts, f_st) -> (m, c), blend(mf, cf, mb, cb, a, t, b) -> m, ones(m) -> confidence
    of a key.  Returns the n planes in frame order."""
    n = len(flows12) + 1
    fwd, bwd, out = {}, {}, [None] * n      # the chains' (mask, confidence) at the frames they have reached
    for steps in plan_mask_propagation(n, keys.keys(), shots):
        for st in steps:
            if st[0] == "key":
                t = st[1]
                fwd[t] = bwd[t] = (keys[t], ones(keys[t]))
                out[t] = keys[t]
            elif st[0] == "step":
                s, t = st[1], st[2]
                if t > s:                                     # forward: the target looks back along flow t -> s
                    fwd[t] = step(fwd[s][0], fwd[s][1], flows21[s], flows12[s])
                    out[t] = fwd[t][0]
                else:
                    bwd[t] = step(bwd[s][0], bwd[s][1], flows12[t], flows21[t])
                    out[t] = bwd[t][0]
            else:
                a, t, b = st[1:]
                out[t] = blend(fwd[t][0], fwd[t][1], bwd[t][0], bwd[t][1], a, t, b)
    return out


def _check_keys(keys, what):
    if not hasattr(keys, "keys") or not len(keys):
        raise ValueError("%s: keys must be a non-empty {frame index: (h, w) float32 mask}" % what)
    keys = {int(k): v for k, v in keys.items()}
    shape = tuple(next(iter(keys.values())).shape)
    for k, v in keys.items():
        if len(v.shape) != 2 or tuple(v.shape) != shape or str(v.dtype) not in ("float32", "torch.float32"):
            raise ValueError("%s: key %d must be a float32 plane %s, got %s %s" % (what, k, shape, tuple(v.shape), v.dtype))
    return keys, shape


def _check_flows(flows12, flows21, shape, what):
    for name, flows in (("flows12", flows12), ("flows21", flows21)):
        for i, f in enumerate(flows):
            if f is not None and (tuple(f.shape) != shape + (2,) or str(f.dtype) not in ("float32", "torch.float32")):
                raise ValueError("%s: %s[%d] must be float32 %s, got %s %s" % (what, name, i, shape + (2,), tuple(f.shape), f.dtype))


def _masks(what, res, keys, flows12, flows21, thresh, shots):
    """The propagation over a residence (_residence.py): numpy through host pointers, or (res None) CUDA tensors on one device."""
    from .atlasfit import load_library, _util_chk
    thresh = _check_thresh(thresh)
    keys, (h, w) = _check_keys(keys, what)
    res = res or one_device(list(keys.values()) + [f for f in list(flows12) + list(flows21) if f is not None],
                            "%s: keys and flows must be CUDA tensors on one device (host arrays go through propagate_masks)" % what)
    keys = {k: res.contiguous(v) for k, v in keys.items()}
    flows12 = [None if f is None else res.contiguous(f) for f in flows12]
    flows21 = [None if f is None else res.contiguous(f) for f in flows21]
    _check_flows(flows12, flows21, (h, w), what)
    shots = _shots_of(flows12, flows21, shots)
    lib, p = load_library(), res.ptr
    res.sync()
    if res.on_device:
        import torch as xp
    else:
        xp = np

    def step(m, c, f_ts, f_st):
        mt, ct = res.empty((h, w), "float32"), res.empty((h, w), "float32")
        _util_chk(lib.af_mask_step(res.ordinal, p(m), p(c), p(f_ts), p(f_st), h, w, thresh, p(mt), p(ct), res.on_device))
        return mt, ct

    def blend(mf, cf, mb, cb, a, t, b):
        o = res.empty((h, w), "float32")
        _util_chk(lib.af_mask_blend(res.ordinal, p(mf), p(cf), p(mb), p(cb), h, w, a, t, b, p(o), res.on_device))
        return o

    return xp.stack(_propagate(keys, flows12, flows21, shots, step, blend, xp.ones_like))


def propagate_masks(keys, flows12, flows21, thresh=DEFAULT_THRESH, shots=None, device=0):
    """Masks of every frame from key masks, through host pointers (the library stages each call on GPU `device`).  keys: {frame index:
    (h, w) float32 in [0, 1]}; flows12[i]: (h, w, 2) float32 flow from frame i to i + 1, flows21[i]: from i + 1 to i, both None at a pair
    across a scene cut.  -> (n, h, w) float32, n = len(flows12) + 1; the key frames are returned untouched."""
    return _masks("propagate_masks", Host(device), keys, flows12, flows21, thresh, shots)


def propagate_masks_device(keys, flows12, flows21, thresh=DEFAULT_THRESH, shots=None):
    """propagate_masks on CUDA tensors (device pointers, no host copy): keys and flows float32 tensors on one device -> an (n, h, w)
    float32 tensor there."""
    return _masks("propagate_masks_device", None, keys, flows12, flows21, thresh, shots)
