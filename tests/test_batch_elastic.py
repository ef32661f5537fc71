"""The host side of the elastic / crop batch (`scene_prep.prepare_batch_store_elastic`), without a GPU: the bound of the crop loop,
the host bound of the noise grids, and the crop draws as a table."""
import numpy as np
import pytest

from d3net_amd import scene_prep as SP
from d3net_amd.config import default_conf


@pytest.mark.parametrize("S", [512, 128, 100, 33, 32, 31, 1])
def test_crop_max_iters_is_the_loop_bound(S):
    """the worst case: the count never drops (n) while every range is > 0; once the x / y range is <= 0 no point can pass"""
    n, calls = 1000, []

    def count(offset, max_pc_range):
        calls.append(max_pc_range.copy())
        return n if (max_pc_range > 0).all() else 0

    _, valid = SP.crop_loop(count, n, np.array([900.0, 700.0, 100.0]), 10, S, np.random.RandomState(0))
    assert valid == 0 and len(calls) == SP.crop_max_iters(S)
    assert (calls[-1][:2] <= 0).all() and (len(calls) == 1 or (calls[-2][:2] > 0).all())


def test_grid_bound_covers_the_real_shape():
    tcfg = default_conf().data.transform
    r = np.random.RandomState(7)
    scale = 50
    gran = SP.elastic_params(scale)[0][0]
    for k in range(200):
        m = SP.augment_matrix(r, tcfg)
        xyz = ((r.rand(1 + k * 3, 3) - r.rand(3)) * r.rand(3) * 12).astype(np.float32)
        s = np.matmul(xyz, m) * scale
        real = SP.grid_shape(np.abs(s).max(0), gran)
        bound = SP.elastic_grid_bound(np.abs(xyz).max(0), m, scale, 0)
        assert bound.dtype == np.int64 and (bound >= real).all(), (k, bound, real)


def test_grid_bound_is_tight():
    """with M = I the bound's value IS |s| max: without the slack cell the bound equals the real shape, with it it is one more"""
    scale = 50
    gran = SP.elastic_params(scale)[0][0]
    for top in (59.99, 60.0, 60.01, 0.0, 399.5):
        xyz = np.array([[top / scale, -0.5, 0.25], [0.1, 0.2, -0.3]], np.float32)
        real = SP.grid_shape(np.abs(np.matmul(xyz, np.eye(3)) * scale).max(0), gran)
        assert np.array_equal(SP.elastic_grid_bound(np.abs(xyz).max(0), np.eye(3), scale, 0, slack=0), real)
        assert np.array_equal(SP.elastic_grid_bound(np.abs(xyz).max(0), np.eye(3), scale, 0), real + 1)


def test_second_bound_adds_the_first_distortion():
    scale = 50
    (g0, m0), (g1, _) = SP.elastic_params(scale)
    a = np.array([4.0, 3.0, 1.5])
    b1 = SP.elastic_grid_bound(a, np.eye(3), scale, 1, slack=0)
    assert np.array_equal(b1, np.floor(a * scale + 6.67 * m0).astype(np.int64) // g1 + 3)


def test_crop_table_rows_are_successive_draws():
    T = SP.crop_max_iters(512)
    assert T == 17
    table = np.random.RandomState(123).rand(T, 3)
    r = np.random.RandomState(123)
    assert np.array_equal(table, np.stack([r.rand(3) for _ in range(T)]))


def test_elastic_enabled_only_in_augmented_detector_mode():
    det = default_conf(overrides={"model": {"no_captioning": True, "no_grounding": True}})
    lis = default_conf(overrides={"model": {"no_captioning": True, "no_grounding": False}})
    assert SP.elastic_enabled(det, True) and not SP.elastic_enabled(det, False) and not SP.elastic_enabled(lis, True)
