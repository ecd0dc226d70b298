"""Host-side pieces of the layer outputs (atlas_outputs.py, tools/make_golden_atlas.py's fixture): no GPU needed."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def atlas_fixture():
    return dict(np.load(os.path.join(GOLDEN, "atlas_seg.npz")))


def test_linspace_restatement_is_torch_bit_for_bit(atlas_fixture):
    """af_render_atlas_texture builds its grid with torch.linspace's fp32 rounding (fma below n // 2, from the end above); the numpy
    restatement of that formula must equal torch.linspace exactly, for the fixture's windows and for random ones."""
    from aiod_amd.atlas_outputs import linspace_f32
    g = atlas_fixture
    cases = [(0.0, 1.0, 1000), (0.0, 1.0, 333)]
    mx, my, e = g["area_bg_scaled"][1], g["area_bg_scaled"][3], g["area_bg_scaled"][4]
    cases += [(mx, np.float32(mx + e), 333), (my, np.float32(my + e), 333), (mx, np.float32(mx + e), 1000)]
    rng = np.random.default_rng(3)
    for _ in range(400):
        s = np.float32(rng.uniform(-1, 1))
        cases.append((s, np.float32(s + np.float32(rng.uniform(-2, 2))), int(rng.choice([1, 2, 7, 64, 333, 500, 1000, 1001]))))
    for s, e_, n in cases:
        want = torch.linspace(float(np.float32(s)), float(np.float32(e_)), n).numpy()
        assert np.array_equal(linspace_f32(s, e_, n), want), (s, e_, n)


def test_normalize_uv_and_uint8_casts():
    from aiod_amd.atlas_outputs import masked_texture, normalize_uv, to_u8
    uv = np.array([[[-1.0, 1.0], [0.2, -0.4]]], np.float32)
    n = normalize_uv(uv, 0.5, 1, 0, 0)                      # fg window (0, 0, 1): u*0.5 + 0.5, clamped to [0, 1]
    assert n.shape == (1, 2, 3) and np.allclose(n[0, :, 0], [0.0, 0.6]) and np.allclose(n[0, :, 1], [1.0, 0.3]) and (n[:, :, 2] == 0).all()
    n2 = normalize_uv(uv, -0.5, np.float32(0.5), np.float32(-1.0), np.float32(-0.5))
    assert np.allclose(n2[0, :, 0], [0.0, 1.0])                            # (-1.0 + 1.0) / 0.5 and (0.1 - 0.5 + 1.0) / 0.5 = 1.2 -> 1
    assert to_u8(np.array([0.999999, 1.0, 0.5])).tolist() == [254, 255, 127]            # truncation, as the reference's astype
    t = np.full((2, 2, 3), 0.5, np.float32)
    assert masked_texture(np.array([[0.0, 1.0], [0.5, 0.002]]), t)[:, :, 0].tolist() == [[0, 127], [63, 0]]


def test_fixture_records_both_alpha_states_and_the_masks_deviation(atlas_fixture):
    g = atlas_fixture
    assert float(g["alpha_scale"]) > 1 and g["checkpoint"] == "ckpt_seg.pt"
    assert g["area_fg_raw"].tolist() == [-1.0, 1.0, -1.0, 1.0, -2.0]        # the reference's empty-selection path
    assert g["area_fg_scaled"][4] > 0 and g["area_bg_scaled"][4] > 0
    a = g["alpha"]
    assert a.min() < 0.1 and a.max() > 0.9                                    # the scaled state spans the alpha range
    m_ref, m_max = g["masks1_ref"], g["masks1_max"]
    assert (m_ref <= m_max).all() and (m_ref != m_max).any()                  # the reference's last-duplicate-wins vs the true maximum
    assert ((m_ref > 0) == (m_max > 0)).all() and set(np.unique(g["masks2"]).tolist()) == {0.0, 1.0}
