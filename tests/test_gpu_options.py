"""uam_set_option / uam_get_option over every name in _lib.OPTIONS: the defaults, that a set
value is the value read back and moves no other option, and that a refused value raises with
the option's UAM_OPT_* name and leaves the stored value alone.

The table below is written from the option switches as they stood before the one option table
replaced them (and from include/uampath.h), not from that table: default, an accepted value
other than the default, a refused value (None: every value is accepted)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

#       name                   default  accepted  refused
TABLE = {
    "group":                  (21,      11,       65),      # G_MAXLEN + 1
    "sorted_min_paths":       (65536,   1000,     -1),
    "k2s_segments":           (2,       4,        9),       # SEG_MAX + 1
    "wave_max_paths":         (16384,   100,      -1),
    "pair_order":             (1,       0,        None),
    "k1_rows":                (2,       4,        3),
    "k3b_segment":            (8,       16,       5),
    "k3b_points_per_lane":    (1,       2,        3),
    "k8_tiled":               (1,       0,        None),
    "k8_streams":             (4,       8,        0),
    "k2g_tile_bits":          (0,       5,        2),
    "k2g_lds_floor":          (0,       54000,    160 * 1024 + 1),
    "k2g_chunk":              (0,       11,       9),
    "k2g_curve":              (1,       0,        2),
    "k2g_sim":                (1,       0,        2),
    "k4h_band":               (0,       4,        3),
    "k2h_lb_stride":          (16,      8,        1025),
    "k2h_terrain":            (1,       0,        2),
    "k4h_terrain":            (0,       1,        2),
    "test_sort_fault":        (0,       1,        2),
    "exact_sum":              (0,       1,        2),
    "exact_sum_volume":       (0,       1,        2),
}
TRUTHY = ("pair_order", "k8_tiled")  # any value is accepted and stored as value != 0


@pytest.fixture()
def eng():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    return Engine(0)


def _all(eng):
    from uam_path_planning_amd import _lib

    return {name: eng.get_option(name) for name in _lib.OPTIONS}


def test_table_covers_every_option():
    from uam_path_planning_amd import _lib

    assert set(TABLE) == set(_lib.OPTIONS)
    assert len(set(_lib.OPTIONS.values())) == len(_lib.OPTIONS)


def test_defaults(eng):
    assert _all(eng) == {name: row[0] for name, row in TABLE.items()}


def test_set_reads_back_and_moves_nothing_else(eng):
    want = {name: row[0] for name, row in TABLE.items()}
    for name, (default, accepted, _) in TABLE.items():
        assert accepted != default
        eng.set_option(name, accepted)
        want[name] = accepted
        assert _all(eng) == want, name
    for name in TRUTHY:
        eng.set_option(name, 5)
        want[name] = 1
        assert _all(eng) == want, name
    # and back to the defaults
    for name, (default, _, _) in TABLE.items():
        eng.set_option(name, default)
        want[name] = default
        assert _all(eng) == want, name


def test_refused_value_names_the_option_and_stores_nothing(eng):
    # at the defaults, and again at the accepted values (a refusal must not reset either)
    for column in (0, 1):
        want = {}
        for name, row in TABLE.items():
            eng.set_option(name, row[column])
            want[name] = row[column]
        for name, row in TABLE.items():
            if row[2] is None:
                continue
            with pytest.raises(ValueError) as err:
                eng.set_option(name, row[2])
            assert "UAM_OPT_" + name.upper() in str(err.value), (name, str(err.value))
            assert _all(eng) == want, name


def test_unknown_key(eng):
    from uam_path_planning_amd import _lib

    before = _all(eng)
    for key in (0, 16, 18, 25, -1, 999):
        assert key not in _lib.OPTIONS.values()
        with pytest.raises(ValueError, match="unknown option"):
            _lib.check(eng.lib.uam_set_option(eng._ctx, key, 1), "uam_set_option")
        v = ctypes.c_int64(-7)
        with pytest.raises(ValueError, match="unknown option"):
            _lib.check(eng.lib.uam_get_option(eng._ctx, key, ctypes.byref(v)), "uam_get_option")
        assert v.value == -7
    assert _all(eng) == before
