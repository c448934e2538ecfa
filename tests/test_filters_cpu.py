"""egonet_amd.filters: the one module that names the filter kinds and maps them to packers (no GPU needed)."""
import pytest
import torch

from egonet_amd import engine, filters, tuner
from egonet_amd.train_common import PackedFilters


def test_kind_names_are_the_values_the_library_returns():
    assert (filters.DIRECT, filters.WINO2, filters.WINO43, filters.WINO4) == (0, 1, 2, 3)
    assert tuner.DIRECT == {filters.DIRECT} and tuner.ALL_KINDS == {0, 1, 2, 3}
    assert sorted(filters.DEVICE_PACK) == [filters.DIRECT, filters.WINO2, filters.WINO4]


def test_engine_reexports_the_host_packers():
    for name in ('pack_conv_weight', 'wino_cot', 'pack_wino_weight', 'pack_wino43_weight', 'pack_wino4_weight',
                 'pack_conv_weight_f16', 'unpack_conv_weight_f16', 'pack_for_kind', 'CK', 'H_CK', 'H_KS'):
        assert getattr(engine, name) is getattr(filters, name), name


@pytest.mark.parametrize('kind', [filters.WINO43, 4, -1, None])
def test_no_device_packer_is_a_value_error_before_anything_is_allocated(kind):
    with pytest.raises(ValueError):
        filters.device_floats(kind, (48, 48, 3, 3), 0)
    pf = PackedFilters(torch.device('cpu'))
    w = torch.zeros(48, 48, 3, 3)
    with pytest.raises(ValueError):
        pf.get(w, 0, None, kind=kind)
    assert pf.entries == {} and pf.table is None


def test_device_floats_refuses_shapes_a_layout_does_not_take():
    assert filters.device_floats(filters.DIRECT, (33, 48, 1, 1), 1) == 3 * 4 * 48 * 4
    assert filters.device_floats(filters.WINO2, (96, 32, 3, 3), 1) == 96 * 32 * 16
    assert filters.device_floats(filters.WINO4, (48, 96, 3, 3), 1) == 96 * 48 * 48
    for kind, shape in ((filters.WINO2, (40, 48, 3, 3)), (filters.WINO2, (48, 48, 1, 1)), (filters.WINO4, (64, 48, 3, 3)),
                        (filters.WINO4, (48, 48, 5, 5))):
        with pytest.raises(ValueError):
            filters.device_floats(kind, shape, 0)
