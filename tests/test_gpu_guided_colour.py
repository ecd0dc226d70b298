"""The guided transfer with a colour guide on the GPU: k_guided_moments, k_guided_solve, k_guided_smooth<9> and
k_guided_apply<.., COLOUR> (csrc/guided.hip) through af_guided_coeffs_colour, af_guided_apply_colour and af_guided_apply_colour16,
guided.py's *_colour functions and Deflicker(proxy_guide="colour"), against the numpy restatement tests/guided_colour_ref.py.

Every comparison is equality, bit for bit: the planes as int32 views, the outputs as samples.  The tolerance is derived, not measured: the
kernels form exact integer sums, then perform single correctly rounded fp64 and fp32 operations in the order include/atlasfit.h writes
out, with contraction off, and the restatement performs the same operations in the same order.

The cases are those of tests/guided_transfer_ref.py (r = 1, 8, 32, windows clipped on both sides, tile boundaries in both directions, the
vector path and the byte tail, 1 x 1 proxies, the largest sums), a grey guide at eps = 64 and at the floor 2^-20 (the worst-conditioned
solve) and a cross-channel colour matrix."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import guided_transfer_ref as G  # noqa: E402
import guided_colour_ref as R  # noqa: E402
import depth_transfer_ref as DT  # noqa: E402
import pipeline_bench as PB  # noqa: E402

DEV = torch.device("cuda", 0)
GREY = tuple("grey_%s_r%d" % (t, r) for t in ("64", "floor") for r in (1, 8, 32))
ALL = G.CASES + GREY + ("matrix",)
DEEP_BITS = (10, 16)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # np.array: a writable copy of a read-only reference


def dev16(a):
    return torch.from_numpy(np.array(a).view(np.int16)).to(DEV).view(torch.uint16)


def host16(t):
    assert t.is_cuda and t.dtype == torch.uint16
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _inputs(name):
    if name in G.CASES:
        return G.make_case(name) + (G.EPS,)
    if name == "matrix":
        return R.make_matrix()[:3] + (8, 64.0)
    _, tag, r = name.split("_")
    return R.make_grey() + (int(r[1:]), 64.0 if tag == "64" else R.EPS_FLOOR)


@pytest.fixture(scope="module")
def reference():
    """The restatement of every case, computed once and never written to: the planes, the 8-bit output, and per depth a deep frame and its
    output."""
    out = {}
    for name in ALL:
        full, i, p, r, eps = _inputs(name)
        A, b = R.coeffs(i, p, r, eps)
        deep = {bits: DT.deepen(full, bits, 7) for bits in DEEP_BITS}
        o16 = {bits: R.apply16(deep[bits], bits, A, b) for bits in DEEP_BITS}
        o = R.apply(full, A, b)
        for arr in (full, i, p, A, b, o) + tuple(deep.values()) + tuple(o16.values()):
            arr.setflags(write=False)
        out[name] = (full, i, p, r, eps, A, b, o, deep, o16)
    return out


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32))


# ---- 1. the restatement, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_host_pointers_match_the_restatement(reference, name):
    import aiod_amd
    full, i, p, r, eps, A_ref, b_ref, o_ref, deep, o16 = reference[name]
    A, b = aiod_amd.guided_coeffs_colour(i, p, radius=r, eps=eps)
    assert A.dtype == np.float32 and b.dtype == np.float32 and A.shape == i.shape[:2] + (9,) and b.shape == i.shape
    assert _same_bits(A, A_ref), (name, np.abs(A - A_ref).max())
    assert _same_bits(b, b_ref), (name, np.abs(b - b_ref).max())
    out = aiod_amd.guided_transfer_colour(full, i, p, radius=r, eps=eps)
    assert out.dtype == np.uint8 and np.array_equal(out, o_ref), (name, int((out != o_ref).sum()))
    assert np.array_equal(aiod_amd.guided_apply_colour(full, A, b), o_ref)
    for bits in DEEP_BITS:
        got = aiod_amd.depth_transfer_colour(deep[bits], bits, i, p, radius=r, eps=eps)
        assert got.dtype == np.uint16 and np.array_equal(got, o16[bits]), (name, bits, int((got != o16[bits]).sum()))
        assert np.array_equal(aiod_amd.guided_apply_colour16(deep[bits], bits, A, b), o16[bits])


@pytest.mark.parametrize("name", ALL)
def test_device_pointers_give_the_same_bytes(reference, name):
    import aiod_amd
    full, i, p, r, eps, A_ref, b_ref, o_ref, deep, o16 = reference[name]
    tf, ti, tp = dev(full), dev(i), dev(p)
    A, b = aiod_amd.guided_coeffs_colour_device(ti, tp, radius=r, eps=eps)
    assert A.is_cuda and b.is_cuda and A.dtype == torch.float32 and tuple(A.shape) == i.shape[:2] + (9,)
    assert _same_bits(A.cpu().numpy(), A_ref) and _same_bits(b.cpu().numpy(), b_ref)
    out = aiod_amd.guided_transfer_colour_device(tf, ti, tp, radius=r, eps=eps)
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), o_ref)
    assert np.array_equal(aiod_amd.guided_apply_colour_device(tf, A, b).cpu().numpy(), o_ref)
    for bits in DEEP_BITS:
        td = dev16(deep[bits])
        got = aiod_amd.depth_transfer_colour_device(td, bits, ti, tp, radius=r, eps=eps)
        assert got.dtype == torch.uint16 and np.array_equal(host16(got), o16[bits]), (name, bits)
        assert np.array_equal(host16(aiod_amd.guided_apply_colour16_device(td, bits, A, b)), o16[bits])
        assert np.array_equal(host16(td), deep[bits])
    assert np.array_equal(tf.cpu().numpy(), full) and np.array_equal(ti.cpu().numpy(), i) and np.array_equal(tp.cpu().numpy(), p)      # inputs untouched


def test_a_work_buffer_of_the_documented_size_gives_the_same_planes(reference):
    """work = 33 h w four-byte words with on_device; nothing past it is written."""
    import aiod_amd
    lib = aiod_amd.load_library()
    _, i, p, r, eps, A_ref, b_ref = reference["tiles"][:7]
    h, w = i.shape[:2]
    ti, tp = dev(i), dev(p)
    A, b = torch.empty((h, w, 9), device=DEV), torch.empty((h, w, 3), device=DEV)
    work = torch.full((33 * h * w + 64,), 7.0, device=DEV)
    torch.cuda.synchronize()
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.af_guided_coeffs_colour(0, q(ti), q(tp), h, w, r, eps, q(A), q(b), q(work), 1) == 0, lib.af_last_error(None).decode()
    assert _same_bits(A.cpu().numpy(), A_ref) and _same_bits(b.cpu().numpy(), b_ref)
    assert (work[33 * h * w:] == 7.0).all().item()


# ---- 2. the identities on the device -----------------------------------------------------------------------------------------------
def test_the_two_identities_on_the_device(reference):
    import aiod_amd
    full, i = reference["ratio"][:2]
    assert np.array_equal(aiod_amd.guided_transfer_colour(full, i, i, radius=8, eps=G.EPS), full)
    rng = np.random.RandomState(3)
    f = rng.randint(70, 186, (75, 106, 3)).astype(np.uint8)
    s = G.area_shrink(f, 37, 53)
    for c in (-37, 60, (5, -9, 21)):
        c = np.broadcast_to(np.array(c, np.int64), (3,))
        pair = (s, (s.astype(np.int64) + c).astype(np.uint8))
        A, b = aiod_amd.guided_coeffs_colour(*pair, radius=8, eps=G.EPS)
        assert not A.any() and np.array_equal(b, np.broadcast_to(c.astype(np.float32), b.shape))
        out = aiod_amd.guided_transfer_colour(f, *pair, radius=8, eps=G.EPS)
        assert np.array_equal(out.astype(np.int64), f.astype(np.int64) + c)


def test_diagonal_planes_give_the_per_channel_bytes(reference):
    """A = diag(a): af_guided_apply's and af_guided_apply16's bytes, on the vector path (r32, wide), the byte path (ratio, w7) and a 1 x 1 proxy."""
    import aiod_amd
    for name in ("r32", "wide", "ratio", "w7", "one"):
        full, i, p, r = reference[name][:4]
        a, b = aiod_amd.guided_coeffs(i, p, radius=r, eps=G.EPS)
        A = np.zeros(a.shape[:2] + (9,), np.float32)
        A[..., 0], A[..., 4], A[..., 8] = a[..., 0], a[..., 1], a[..., 2]
        assert np.array_equal(aiod_amd.guided_apply_colour(full, A, b), aiod_amd.guided_apply(full, a, b)), name
        for bits in DEEP_BITS:
            deep = reference[name][8][bits]
            assert np.array_equal(aiod_amd.guided_apply_colour16(deep, bits, A, b), aiod_amd.guided_apply16(deep, bits, a, b)), (name, bits)


def test_deep_apply_at_8_bits_and_at_16(reference):
    import aiod_amd
    for name in ("ratio", "same", "one", "wide", "r32", "matrix"):      # 8 bits on widened bytes: af_guided_apply_colour's bytes
        full, _, _, _, _, A, b, o_ref = reference[name][:8]
        assert np.array_equal(aiod_amd.guided_apply_colour16(full.astype(np.uint16), 8, A, b), o_ref), name
    rng = np.random.default_rng(9)
    zero = np.zeros((5, 7, 9), np.float32)
    full = rng.integers(37 * 257, 65536 - 60 * 257, (13, 16, 3)).astype(np.uint16)      # 16 bits, A = 0, b = c: F + 257 c where nothing clips
    for c in (-37, 1, 60):
        out = aiod_amd.guided_apply_colour16(full, 16, zero, np.full((5, 7, 3), c, np.float32))
        assert np.array_equal(out.astype(np.int64), full.astype(np.int64) + 257 * c)


# ---- 3. misaligned pointers --------------------------------------------------------------------------------------------------------
def test_misaligned_device_pointers_take_the_byte_path(reference):
    """W a multiple of 4 but the frame one byte off a 4-byte boundary (the deep frame 2 bytes off an 8-byte one): the same bytes."""
    import aiod_amd
    for name in ("r32", "w8", "w8_one"):
        full, i, p, r, eps, A, b, o_ref, deep, o16 = reference[name]
        assert full.shape[1] % 4 == 0
        buf = torch.zeros(full.size + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = dev(full).reshape(-1)
        tf = buf[1:].view(full.shape)
        assert tf.data_ptr() % 4 == 1 and tf.is_contiguous()
        out = aiod_amd.guided_transfer_colour_device(tf, dev(i), dev(p), radius=r, eps=eps)
        assert np.array_equal(out.cpu().numpy(), o_ref), name
        td = dev16(np.concatenate([[0], deep[10].reshape(-1)]).astype(np.uint16))[1:].view(full.shape)
        assert td.data_ptr() % 8 == 2 and td.is_contiguous()
        assert np.array_equal(host16(aiod_amd.guided_apply_colour16_device(td, 10, dev(A), dev(b))), o16[10]), name


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_each_refusal_carries_its_message_and_writes_nothing():
    import aiod_amd
    lib = aiod_amd.load_library()
    u8 = torch.zeros((4, 6, 3), dtype=torch.uint8, device=DEV)
    pa, pb = torch.full((4, 6, 9), 7.0, device=DEV), torch.full((4, 6, 3), 7.0, device=DEV)
    big, out = torch.zeros((8, 12, 3), dtype=torch.uint8, device=DEV), torch.full((8, 12, 3), 7, dtype=torch.uint8, device=DEV)
    big16, out16 = torch.zeros((8, 12, 3), dtype=torch.int16, device=DEV), torch.full((8, 12, 3), 7, dtype=torch.int16, device=DEV)
    work = torch.full((33 * 4 * 6,), 7.0, device=DEV)
    q = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    torch.cuda.synchronize()

    def coeffs(h=4, w=6, r=8, eps=64.0, b=pb, wk=None):
        return lib.af_guided_coeffs_colour(0, q(u8), q(u8), h, w, r, eps, q(pa), q(b), None if wk is None else q(wk), 1)

    def apply(H=8, W=12, h=4, w=6, o=out):
        return lib.af_guided_apply_colour(0, q(big), H, W, q(pa), q(pb), h, w, q(o), 1)

    def apply16(H=8, W=12, bits=10, o=out16, off=0):
        return lib.af_guided_apply_colour16(0, q(big16), H, W, bits, q(pa), q(pb), 4, 6, q(o, off), 1)

    for call, msg in ((lambda: coeffs(r=0), "af_guided_coeffs_colour: r must be 1..32"),
                      (lambda: coeffs(r=33), "af_guided_coeffs_colour: r must be 1..32"),
                      (lambda: coeffs(eps=0.0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(eps=2.0 ** -21), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(eps=float("inf")), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(h=0), "af_guided_coeffs_colour: h must be 1..16384"),
                      (lambda: coeffs(w=16385), "af_guided_coeffs_colour: w must be 1..16384"),
                      (lambda: coeffs(b=pa), "af_guided_coeffs_colour: a_out aliases b_out"),
                      (lambda: coeffs(wk=pa), "af_guided_coeffs_colour: work aliases an output"),
                      (lambda: apply(H=16385), "af_guided_apply_colour: H must be 1..16384"),
                      (lambda: apply(W=0), "af_guided_apply_colour: W must be 1..16384"),
                      (lambda: apply(H=3), "af_guided_apply_colour: the proxy is larger than the full frame"),
                      (lambda: apply(o=big), "af_guided_apply_colour: the output aliases an input"),
                      (lambda: apply16(bits=17), "af_guided_apply_colour16: bits must be 8..16"),
                      (lambda: apply16(off=1), "af_guided_apply_colour16: uint16 pointers must be 2-byte aligned"),
                      (lambda: apply16(o=big16), "af_guided_apply_colour16: the output aliases an input")):
        assert call() == -1, msg
        assert lib.af_last_error(None).decode() == msg
    assert (pa == 7).all().item() and (pb == 7).all().item() and (out == 7).all().item() and (out16 == 7).all().item()
    assert coeffs(eps=2.0 ** -20, wk=work) == 0 and apply() == 0 and apply16() == 0      # and the same buffers, argued properly, are accepted


# ---- 5. the pipeline ---------------------------------------------------------------------------------------------------------------
H, W, DOWN, SEED, N, EDGE, RADIUS, DEPTH = 130, 197, 4, 11, 3, 195, 5, 10      # the smallest clip of tests/test_gpu_deflicker_proxy.py
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


@pytest.fixture(scope="module")
def clip():
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    from aiod_amd.preprocess_optical_flow import shrink_size
    import aiod_amd
    weights = PB.synthetic_weights()
    cfg = dict(REFERENCE_CONFIG, **SHORT)

    def run(frames, run_kw=None, **kw):
        return aiod_amd.Deflicker(*weights, config=cfg, down=DOWN, seed=SEED, **kw).run(frames, **(run_kw or {}))
    return {"frames": PB.synthetic_clip(N, H, W, seed=5), "run": run, "small": shrink_size(H, W, EDGE)}


def test_proxy_route_with_the_colour_guide_is_the_plain_run_carried_up_by_it(clip):
    import aiod_amd
    frames, run, (h, w) = clip["frames"], clip["run"], clip["small"]
    res = run(frames, proxy_long_edge=EDGE, proxy_radius=RADIUS, proxy_guide="colour")
    assert res["final"].shape == (N, H, W, 3) and res["final"].dtype == np.uint8
    assert res["proxy"] == {"size": [h, w], "radius": RADIUS, "eps": aiod_amd.DEFAULT_EPS, "guide": "colour"}
    small = [aiod_amd.resize_area(f, h, w) for f in frames]
    plain = run(small)
    differs = False
    for i in range(N):
        expect = aiod_amd.guided_transfer_colour(frames[i], small[i], plain["final"][i], radius=RADIUS, eps=aiod_amd.DEFAULT_EPS)
        assert np.array_equal(res["final"][i], expect), (i, int((res["final"][i] != expect).sum()))
        differs |= not np.array_equal(expect, aiod_amd.guided_transfer(frames[i], small[i], plain["final"][i], radius=RADIUS, eps=aiod_amd.DEFAULT_EPS))
    assert differs                                            # the guide was not the default's


def test_deep_route_with_the_colour_guide_is_the_plain_run_carried_to_the_deep_frames(clip):
    import aiod_amd
    frames, run, (h, w) = clip["frames"], clip["run"], clip["small"]
    rng = np.random.default_rng(17)
    deep = [(4 * f.astype(np.uint16) + rng.integers(0, 4, f.shape).astype(np.uint16)).astype(np.uint16) for f in frames]
    res = run(deep, run_kw={"bits": DEPTH}, proxy_long_edge=EDGE, proxy_radius=RADIUS, proxy_guide="colour")
    assert res["final"].shape == (N, H, W, 3) and res["final"].dtype == np.uint16
    assert res["depth"] == {"bits": DEPTH, "radius": RADIUS, "eps": aiod_amd.DEFAULT_EPS, "guide": "colour"} and res["proxy"]["guide"] == "colour"
    small = [aiod_amd.resize_area(aiod_amd.reduce_depth(f, DEPTH), h, w) for f in deep]
    plain = run(small)
    for i in range(N):
        expect = aiod_amd.depth_transfer_colour(deep[i], DEPTH, small[i], plain["final"][i], radius=RADIUS, eps=aiod_amd.DEFAULT_EPS)
        assert np.array_equal(res["final"][i], expect), (i, int((res["final"][i] != expect).sum()))


def test_the_default_guide_by_name_is_the_run_without_the_keyword(clip):
    frames, run = clip["frames"], clip["run"]
    named = run(frames, proxy_long_edge=EDGE, proxy_radius=RADIUS, proxy_guide="channel")
    without = run(frames, proxy_long_edge=EDGE, proxy_radius=RADIUS)
    assert np.array_equal(named["final"], without["final"])
    assert named["proxy"] == without["proxy"] and "guide" not in named["proxy"] and list(named) == list(without)
