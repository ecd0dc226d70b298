"""af_mask_step / af_mask_blend and masks.propagate_masks on the GPU against the numpy restatement tests/maskprop_ref.py.

Every comparison is bit for bit: the kernels (csrc/maskprop.hip) perform single correctly rounded fp32 operations with contraction off,
in the order the restatement performs them, the division is HIP's correctly rounded one, and no operation depends on an order of
summation.  A difference is a bug, not a tolerance to widen."""
import ctypes as C

import numpy as np
import pytest
import torch

import maskprop_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1), (1, 37), (41, 1), (67, 41), (130, 259)]      # partial 64 x 4 workgroups on both axes, more than one of each


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    assert got.dtype == want.dtype == F and got.shape == want.shape
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s differs at %d of %d pixels, first %s: %r vs %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]),
                                                                               got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def _flow_cases(h, w, rng):
    """{name: (f_ts, f_st, thresh)} covering both branches of both tests of the kernel."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = lambda: np.zeros((h, w, 2), F)      # noqa: E731
    cases = {}
    f_ts = rng.uniform(-2.5, 2.5, (h, w, 2)).astype(F)
    cases["random sub-pixel"] = (f_ts, (-f_ts + rng.uniform(-0.9, 0.9, (h, w, 2))).astype(F), 1.0)      # round-trip norms on both sides of 1
    f_ts = rng.integers(-3, 4, (h, w, 2)).astype(F)
    cases["integer"] = (f_ts, (-f_ts + rng.integers(-1, 2, (h, w, 2)) * (rng.random((h, w, 2)) < 0.2)).astype(F), 0.75)
    f_ts = z()                                               # every pixel lands exactly on the last column and row: x1 and y1 are clamped
    f_ts[..., 0], f_ts[..., 1] = (w - 1) - xs, (h - 1) - ys
    f_st = rng.uniform(-0.5, 0.5, (h, w, 2)).astype(F)
    cases["onto w-1 / h-1"] = (f_ts, f_st, 1.0)              # one source pixel for all: only the targets next to it close their round trip
    cases["onto w-1 / h-1, all consistent"] = (f_ts, f_st, 2.0 * (h + w))
    f_ts = z()                                               # onto the last column in the pixel's own row, then onto the last row in its own column
    f_ts[: h // 2 + 1, :, 0], f_ts[h // 2 + 1:, :, 1] = ((w - 1) - xs)[: h // 2 + 1], ((h - 1) - ys)[h // 2 + 1:]
    cases["onto w-1 or h-1"] = (f_ts, f_st, 3.0)
    f_ts = z()                                               # the border pixels leave the frame on their own side by a fraction, the rest stay
    f_ts[:, 0, 0], f_ts[:, w - 1, 0], f_ts[0, :, 1], f_ts[h - 1, :, 1] = -0.25, 0.25, -0.5, 0.5
    f_ts[h // 2, w // 2] = (-float(w), 0)
    f_ts[h // 3, w // 3] = (0, float(h))
    cases["leaving on each side"] = (f_ts, -f_ts, 1.0)
    f_ts, f_st = rng.uniform(-1, 1, (h, w, 2)).astype(F), rng.uniform(-1, 1, (h, w, 2)).astype(F)
    bad = np.array([np.nan, np.inf, -np.inf, -0.0], F)
    f_ts[rng.random((h, w, 2)) < 0.1] = 0
    f_ts[..., 0].flat[::5] = bad[np.arange(len(f_ts[..., 0].flat[::5])) % 4]
    f_ts[..., 1].flat[3::7] = bad[np.arange(len(f_ts[..., 1].flat[3::7])) % 4]
    f_st[..., 0].flat[2::11] = bad[np.arange(len(f_st[..., 0].flat[2::11])) % 4]
    cases["NaN and inf"] = (f_ts, f_st, 1.0)
    f_ts = z()                                               # zero look-up, round trips of norm thresh -+ a few ulps and exactly thresh
    f_st = z()
    r = (F(1) + (rng.integers(-3, 4, (h, w)) * F(2 ** -23))).astype(F)
    ang = rng.integers(0, 4, (h, w))
    f_st[..., 0], f_st[..., 1] = np.where(ang % 2 == 0, r * (1 - ang), 0), np.where(ang % 2 == 1, r * (2 - ang), 0)
    cases["straddling thresh"] = (f_ts, f_st.astype(F), 1.0)
    return cases


def _step(m_s, c_s, f_ts, f_st, thresh, on_device):
    import aiod_amd
    lib = aiod_amd.load_library()
    h, w = m_s.shape
    if not on_device:
        m_t, c_t = np.full((h, w), 7, F), np.full((h, w), 7, F)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        rc = lib.af_mask_step(0, p(m_s), p(c_s), p(f_ts), p(f_st), h, w, thresh, p(m_t), p(c_t), 0)
        assert rc == 0, lib.af_last_error(None).decode()
        return m_t, c_t
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m_s, c_s, f_ts, f_st)]
    m_t, c_t = torch.full((h, w), 7.0, device="cuda"), torch.full((h, w), 7.0, device="cuda")
    torch.cuda.synchronize()
    rc = lib.af_mask_step(0, *[C.c_void_p(x.data_ptr()) for x in t], h, w, thresh, C.c_void_p(m_t.data_ptr()), C.c_void_p(c_t.data_ptr()), 1)
    assert rc == 0, lib.af_last_error(None).decode()
    return m_t.cpu().numpy(), c_t.cpu().numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_step_equals_the_restatement_bit_for_bit(h, w):
    rng = np.random.default_rng(100 * h + w)
    m_s, c_s = rng.random((h, w)).astype(F), rng.random((h, w)).astype(F)
    c_s[rng.random((h, w)) < 0.2] = 0
    m_s[rng.random((h, w)) < 0.2] = 1
    for name, (f_ts, f_st, thresh) in _flow_cases(h, w, rng).items():
        f_ts, f_st = np.ascontiguousarray(f_ts, F), np.ascontiguousarray(f_st, F)
        want_m, want_c = R.step(m_s, c_s, f_ts, f_st, thresh)
        if h * w >= 67 * 41 and name in ("random sub-pixel", "integer", "straddling thresh", "NaN and inf"):      # the case does exercise both branches
            assert 0 < (want_c == 0).sum() and (want_c > 0).sum() > 0, name
        for on_device in (False, True):
            got_m, got_c = _step(m_s, c_s, f_ts, f_st, thresh, on_device)
            _same(got_m, want_m, "%s m_t (%s pointers)" % (name, "device" if on_device else "host"))
            _same(got_c, want_c, "%s c_t (%s pointers)" % (name, "device" if on_device else "host"))
    if (h, w) == (67, 41):      # the named edge pixels of the border case, so that the case cannot pass by holding everything
        f_ts, f_st, _ = _flow_cases(h, w, np.random.default_rng(0))["leaving on each side"]
        _, c = R.step(m_s, np.ones((h, w), F), f_ts, f_st)
        assert (c[:, 0] == 0).all() and (c[:, w - 1] == 0).all() and (c[0] == 0).all() and (c[h - 1] == 0).all() and c[h // 2, w // 2] == 0
        assert (c[1:h - 1, 1:w - 1] == 1).sum() == (h - 2) * (w - 2) - 2
        f_ts, f_st, big = _flow_cases(h, w, np.random.default_rng(0))["onto w-1 / h-1, all consistent"]
        m, c = R.step(m_s, np.ones((h, w), F), f_ts, f_st, big)
        assert (c == 1).all() and (m == m_s[h - 1, w - 1]).all()
        _, c = R.step(m_s, np.ones((h, w), F), f_ts, f_st, 1.0)
        assert c[h - 1, w - 1] == 1 and c[0, 0] == 0


def test_blend_equals_the_restatement_bit_for_bit():
    import aiod_amd
    lib = aiod_amd.load_library()
    h, w = 67, 41
    rng = np.random.default_rng(7)
    m_f, c_f, m_b, c_b = (rng.random((h, w)).astype(F) for _ in range(4))
    c_f[rng.random((h, w)) < 0.3] = 0
    c_b[rng.random((h, w)) < 0.3] = 0
    c_f[5], c_b[5] = 0, 0                                    # neither chain has confidence: the distance-weighted mean
    m_f[7], m_b[7] = 1.5, 1.25                               # out of range on purpose: the result needs the clamp
    m_f[8], m_b[8] = -0.5, -0.25
    m_f[9, :5] = np.nan
    for a, t, b in ((0, 1, 2), (3, 4, 11), (0, 6, 7), (10, 1000, 70000)):
        want = R.blend(m_f, c_f, m_b, c_b, a, t, b)
        assert (want[7] == 1).all() and (want[8] == 0).all() and ((c_f == 0) & (c_b == 0)).sum() > w and np.isnan(want[9, :5]).all()
        out = np.full((h, w), 7, F)
        p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
        assert lib.af_mask_blend(0, p(m_f), p(c_f), p(m_b), p(c_b), h, w, a, t, b, p(out), 0) == 0, lib.af_last_error(None).decode()
        assert np.array_equal(np.isnan(out), np.isnan(want))
        _same(np.nan_to_num(out, nan=-1), np.nan_to_num(want, nan=-1), "blend %s (host pointers)" % ((a, t, b),))
        dev = [torch.from_numpy(x).cuda() for x in (m_f, c_f, m_b, c_b)]
        o = torch.full((h, w), 7.0, device="cuda")
        torch.cuda.synchronize()
        assert lib.af_mask_blend(0, *[C.c_void_p(x.data_ptr()) for x in dev], h, w, a, t, b, C.c_void_p(o.data_ptr()), 1) == 0
        _same(np.nan_to_num(o.cpu().numpy(), nan=-1), np.nan_to_num(want, nan=-1), "blend %s (device pointers)" % ((a, t, b),))


@pytest.fixture(scope="module")
def clip():
    """7 frames of 40 x 24: smooth flows of a pixel or two with rough spots, so that chains lose and keep confidence."""
    rng = np.random.default_rng(11)
    n, h, w = 7, 24, 40
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f12, f21 = [], []
    for i in range(n - 1):
        f = np.stack([1.3 + 0.4 * np.sin(ys / 5.0 + i), -0.6 + 0.3 * np.cos(xs / 7.0 - i)], -1)
        f12.append((f + rng.uniform(-0.2, 0.2, f.shape)).astype(F))
        back = -f + rng.uniform(-0.2, 0.2, f.shape)
        back[rng.random((h, w)) < 0.1] += 2.0
        f21.append(back.astype(F))
    key = lambda cx, cy: np.clip(1.5 - np.hypot(xs - cx, ys - cy) / 5.0, 0, 1).astype(F)      # noqa: E731
    return {"n": n, "f12": f12, "f21": f21, "keys": {0: key(12, 14), 3: key(17, 12), 6: key(22, 10)}}


@pytest.mark.parametrize("which", [(0, 6), (3,), (0, 3, 6)])
def test_propagation_equals_the_restatements_loop(clip, which):
    import aiod_amd
    keys = {k: clip["keys"][k] for k in which}
    want = R.propagate(keys, clip["f12"], clip["f21"])
    assert want.shape == (7, 24, 40) and ((want > 0) & (want < 1)).any()
    host = aiod_amd.propagate_masks(keys, clip["f12"], clip["f21"])
    _same(host, want, "propagate_masks keys %s" % (which,))
    cu = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    dev = aiod_amd.propagate_masks_device({k: cu(v) for k, v in keys.items()}, [cu(f) for f in clip["f12"]], [cu(f) for f in clip["f21"]])
    assert dev.is_cuda and dev.dtype == torch.float32
    _same(dev.cpu().numpy(), want, "propagate_masks_device keys %s" % (which,))
    for k in which:
        assert np.array_equal(host[k], keys[k])              # key frames are returned untouched
    if which == (0, 6):
        other = aiod_amd.propagate_masks(keys, clip["f12"], clip["f21"], thresh=0.25)
        _same(other, R.propagate(keys, clip["f12"], clip["f21"], 0.25), "thresh 0.25")
        assert not np.array_equal(other, host)


def test_propagation_never_crosses_a_cut(clip):
    """A cut at pair 3: each shot is the propagation of its own frames, flows and key, indices shifted."""
    import aiod_amd
    f12, f21 = list(clip["f12"]), list(clip["f21"])
    f12[3] = f21[3] = None
    keys = {1: clip["keys"][0], 6: clip["keys"][6]}
    got = aiod_amd.propagate_masks(keys, f12, f21)
    a = aiod_amd.propagate_masks({1: keys[1]}, f12[:3], f21[:3])
    b = aiod_amd.propagate_masks({2: keys[6]}, f12[4:], f21[4:])
    _same(got, np.concatenate([a, b]), "two shots")
    _same(got, aiod_amd.propagate_masks(keys, f12, f21, shots=[(0, 4), (4, 7)]), "explicit shots")
    with pytest.raises(ValueError, match=r"shot 1 \(frames 4\.\.6\) holds no key mask"):
        aiod_amd.propagate_masks({1: keys[1]}, f12, f21)
    with pytest.raises(ValueError, match="pair 3 inside shot 0..6 has no flow"):
        aiod_amd.propagate_masks(keys, f12, f21, shots=[(0, 7)])


def test_einval_cases_name_the_cause_and_leave_the_outputs_untouched():
    import aiod_amd
    lib = aiod_amd.load_library()
    h, w = 6, 9
    m, c, o1, o2 = (np.full((h, w), v, F) for v in (0.5, 1.0, 7.0, 7.0))
    f = np.zeros((2, h, w, 2), F)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731

    def step(args, msg):
        rc = lib.af_mask_step(0, *[p(x) if isinstance(x, (np.ndarray, type(None))) else x for x in args], 0)
        text = lib.af_last_error(None).decode()
        assert rc == -1 and text == "af_mask_step: " + msg, (rc, text)      # AF_EINVAL
        assert (o1 == 7).all() and (o2 == 7).all() and (m == 0.5).all()

    step((None, c, f[0], f[1], h, w, 1.0, o1, o2), "null pointer")
    step((m, c, f[0], f[1], h, w, 1.0, o1, None), "null pointer")
    step((m, c, f[0], f[1], 0, w, 1.0, o1, o2), "h must be 1..16384")
    step((m, c, f[0], f[1], h, 16385, 1.0, o1, o2), "w must be 1..16384")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        step((m, c, f[0], f[1], h, w, bad, o1, o2), "thresh must be finite and > 0")
    step((m, c, f[0], f[1], h, w, 1.0, m, o2), "an output aliases an input")
    step((m, c, f[0], f[1], h, w, 1.0, o1, f[1].reshape(-1)[h * w:].reshape(h, w)), "an output aliases an input")      # overlaps, starts elsewhere
    step((m, c, f[0], f[1], h, w, 1.0, o1, o1), "m_t aliases c_t")

    def blend(args, msg):
        rc = lib.af_mask_blend(0, *[p(x) if isinstance(x, (np.ndarray, type(None))) else x for x in args], 0)
        text = lib.af_last_error(None).decode()
        assert rc == -1 and text == "af_mask_blend: " + msg, (rc, text)
        assert (o1 == 7).all() and (m == 0.5).all()

    blend((m, c, m, None, h, w, 0, 1, 2, o1), "null pointer")
    blend((m, c, m, c, 16385, w, 0, 1, 2, o1), "h must be 1..16384")
    blend((m, c, m, c, h, 0, 0, 1, 2, o1), "w must be 1..16384")
    for a, t, b in ((0, 0, 2), (0, 2, 2), (2, 1, 0), (1, 0, 2)):
        blend((m, c, m, c, h, w, a, t, b, o1), "frames must satisfy a < t < b")
    blend((m, c, m, c, h, w, 0, 1, 2, c), "the output aliases an input")
    with pytest.raises(aiod_amd.AtlasFitError, match="af_mask_step: thresh"):
        aiod_amd.propagate_masks({0: m}, [f[0]], [f[1]], thresh=1e-320)      # positive in fp64, 0 as the ABI's float: the library's own refusal
    with pytest.raises(ValueError, match="thresh must be finite and > 0"):
        aiod_amd.propagate_masks({0: m}, [f[0]], [f[1]], thresh=0)
    with pytest.raises(ValueError, match=r"flows12\[0\] must be float32 \(6, 9, 2\)"):
        aiod_amd.propagate_masks({0: m}, [f[0][:5]], [f[1]])
    with pytest.raises(ValueError, match="must be CUDA tensors on one device"):
        aiod_amd.propagate_masks_device({0: torch.from_numpy(m)}, [torch.from_numpy(f[0])], [torch.from_numpy(f[1])])
    got = aiod_amd.propagate_masks({0: m}, [f[0]], [f[1]])   # and the library still works
    assert np.array_equal(got, np.stack([m, m]))
