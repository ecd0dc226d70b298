"""af_guided_coeffs / af_guided_apply and guided.py on the GPU against the numpy restatement tests/guided_transfer_ref.py.

Every comparison is equality, bit for bit: the coefficient planes as int32 views, the output as bytes.  The tolerance is derived, not
measured: the kernels form exact integer sums and then perform single correctly rounded fp32 (fp64 for the tap positions) operations in
one documented order with contraction off, and the restatement performs the same operations in the same order.

The cases (guided_transfer_ref.make_case) are the smallest at which the kernels can still go wrong: a non-integer ratio; ratio 1, where
the taps coincide; r = 1, 8 and 32, the last on a 37-row proxy so the window is clipped on both sides; a 70 x 131 proxy at r = 5, which
crosses the 32 x 16 tiles in both directions with a width that is no multiple of 64; a 1 x 1 proxy under a 2 x 3 frame; I = 255, P = 0 on a
70 x 70 proxy at r = 32 (the largest sums: pins the int32 claim); I = P; random bytes; full widths that are (200, 516: the 12-byte
path, 516 spanning two workgroups) and are not multiples of 4; and 5-row frames of W = 8 and W = 7 (the tail of a group of four) over
3 x 2 and 1 x 1 proxies, the W = 8 ones also as a view one byte into a buffer."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_transfer_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def reference():
    """The restatement of every case, computed once and never written to."""
    out = {}
    for name in R.CASES:
        full, i, p, r = R.make_case(name)
        a, b = R.coeffs(i, p, r, R.EPS)
        o = R.apply(full, a, b)
        for arr in (full, i, p, a, b, o):
            arr.setflags(write=False)
        out[name] = (full, i, p, r, a, b, o)
    return out


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32))


@pytest.mark.parametrize("name", R.CASES)
def test_host_pointers_match_the_restatement(reference, name):
    import aiod_amd
    full, i, p, r, a_ref, b_ref, o_ref = reference[name]
    a, b = aiod_amd.guided_coeffs(i, p, radius=r, eps=R.EPS)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert _same_bits(a, a_ref), (name, np.abs(a - a_ref).max())
    assert _same_bits(b, b_ref), (name, np.abs(b - b_ref).max())
    out = aiod_amd.guided_transfer(full, i, p, radius=r, eps=R.EPS)
    assert out.dtype == np.uint8 and np.array_equal(out, o_ref), (name, int((out != o_ref).sum()))


@pytest.mark.parametrize("name", R.CASES)
def test_device_pointers_give_the_same_bytes(reference, name):
    import aiod_amd
    full, i, p, r, a_ref, b_ref, o_ref = reference[name]
    dev = torch.device("cuda", 0)
    tf, ti, tp = (torch.from_numpy(np.array(x)).to(dev) for x in (full, i, p))
    a, b = aiod_amd.guided_coeffs_device(ti, tp, radius=r, eps=R.EPS)
    assert a.is_cuda and b.is_cuda and a.dtype == torch.float32
    assert _same_bits(a.cpu().numpy(), a_ref) and _same_bits(b.cpu().numpy(), b_ref)
    out = aiod_amd.guided_transfer_device(tf, ti, tp, radius=r, eps=R.EPS)
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), o_ref)
    assert np.array_equal(tf.cpu().numpy(), full) and np.array_equal(ti.cpu().numpy(), i) and np.array_equal(tp.cpu().numpy(), p)      # inputs untouched


def test_the_two_identities_on_the_device(reference):
    import aiod_amd
    full, i, _, _, _, _, _ = reference["ratio"]
    assert np.array_equal(aiod_amd.guided_transfer(full, i, i, radius=8, eps=R.EPS), full)
    rng = np.random.RandomState(3)
    f = rng.randint(70, 186, (75, 106, 3)).astype(np.uint8)
    s = R.area_shrink(f, 37, 53)
    for c in (-37, 60):
        out = aiod_amd.guided_transfer(f, s, (s.astype(np.int64) + c).astype(np.uint8), radius=8, eps=R.EPS)
        assert np.array_equal(out.astype(np.int64), f.astype(np.int64) + c)


def test_misaligned_device_pointers_take_the_byte_path(reference):
    """W a multiple of 4 but the frame and the output one byte off a 4-byte boundary: the same bytes through the byte path."""
    import aiod_amd
    for name in ("r32", "w8", "w8_one"):
        full, i, p, r, _, _, o_ref = reference[name]
        assert full.shape[1] % 4 == 0
        dev = torch.device("cuda", 0)
        buf = torch.zeros(full.size + 1, dtype=torch.uint8, device=dev)
        buf[1:] = torch.from_numpy(np.array(full)).to(dev).reshape(-1)
        tf = buf[1:].view(full.shape)
        assert tf.data_ptr() % 4 == 1 and tf.is_contiguous()
        out = aiod_amd.guided_transfer_device(tf, torch.from_numpy(np.array(i)).to(dev), torch.from_numpy(np.array(p)).to(dev), radius=r, eps=R.EPS)
        assert np.array_equal(out.cpu().numpy(), o_ref), name


def test_each_refusal_carries_its_message():
    import ctypes as C
    import aiod_amd
    lib = aiod_amd.load_library()
    dev = torch.device("cuda", 0)
    u8 = torch.zeros((4, 6, 3), dtype=torch.uint8, device=dev)
    pa, pb = torch.zeros((4, 6, 3), device=dev), torch.zeros((4, 6, 3), device=dev)
    big, out = torch.zeros((8, 12, 3), dtype=torch.uint8, device=dev), torch.zeros((8, 12, 3), dtype=torch.uint8, device=dev)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    torch.cuda.synchronize()

    def coeffs(h=4, w=6, r=8, eps=64.0, b=pb):
        return lib.af_guided_coeffs(0, q(u8), q(u8), h, w, r, eps, q(pa), q(b), None, 1)

    def apply(H=8, W=12, h=4, w=6, o=out):
        return lib.af_guided_apply(0, q(big), H, W, q(pa), q(pb), h, w, q(o), 1)

    for call, msg in ((lambda: coeffs(r=0), "af_guided_coeffs: r must be 1..32"),
                      (lambda: coeffs(r=33), "af_guided_coeffs: r must be 1..32"),
                      (lambda: coeffs(eps=0.0), "af_guided_coeffs: eps must be finite and > 0"),
                      (lambda: coeffs(eps=float("inf")), "af_guided_coeffs: eps must be finite and > 0"),
                      (lambda: coeffs(h=0), "af_guided_coeffs: h must be 1..16384"),
                      (lambda: coeffs(w=16385), "af_guided_coeffs: w must be 1..16384"),
                      (lambda: coeffs(b=pa), "af_guided_coeffs: a_out aliases b_out"),
                      (lambda: apply(H=16385), "af_guided_apply: H must be 1..16384"),
                      (lambda: apply(W=0), "af_guided_apply: W must be 1..16384"),
                      (lambda: apply(H=3), "af_guided_apply: the proxy is larger than the full frame"),
                      (lambda: apply(o=big), "af_guided_apply: the output aliases an input")):
        assert call() == -1, msg
        assert lib.af_last_error(None).decode() == msg
    assert coeffs() == 0 and apply() == 0      # and the same buffers, argued properly, are accepted
