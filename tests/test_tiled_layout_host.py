"""The tiled device layout (include/ocs.h, ocs_integrator_set_layout), host side: the NumPy index map is the formula of the
header and a bijection onto the non-pad positions, ocs_tiled_doubles agrees with it, and the new symbols are exported with the
declared signatures.  No GPU needed."""
import ctypes as C
import re

import numpy as np
import pytest

ROWS, COLS, BATCHES = (1, 5), (1, 9), (1, 15, 16, 17, 70)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("batch", BATCHES)
def test_tiled_index_is_the_formula_and_a_bijection(pkg, rows, cols, batch):
    ix = pkg.tiled_index(rows, cols, batch)
    assert ix.shape == (cols, rows, batch) and ix.dtype == np.int64
    for i in range(cols):
        for r in range(rows):
            for b in range(batch):
                assert ix[i, r, b] == ((b // 16) * cols + i) * rows * 16 + r * 16 + (b % 16)
    n = pkg.tiled_doubles(rows, cols, batch)
    tiles = -(-batch // 16)
    assert n == tiles * 16 * rows * cols
    flat = ix.ravel()
    assert flat.min() >= 0 and flat.max() < n and np.unique(flat).size == flat.size
    # the positions it does not reach are exactly the pad lanes of the last tile
    pad = np.setdiff1d(np.arange(n), flat)
    assert pad.size == (tiles * 16 - batch) * rows * cols
    assert np.all(pad // (rows * cols * 16) == tiles - 1) and np.all(pad % 16 >= batch - (tiles - 1) * 16)


def test_new_symbols_are_exported_with_the_declared_signatures(pkg):
    from ocs_amd import _lib
    vp, ci = C.c_void_p, C.c_int
    want = {
        "ocs_integrator_set_layout": ("int", C.c_int, [vp, ci]),
        "ocs_integrator_layout": ("int", C.c_int, [vp]),
        "ocs_to_tiled_dev": ("int", C.c_int, [vp, vp, ci, ci, ci, vp]),
        "ocs_from_tiled_dev": ("int", C.c_int, [vp, vp, ci, ci, ci, vp]),
        "ocs_tiled_doubles": ("long", C.c_long, [ci, ci, ci]),
    }
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, (ret, res, args) in want.items():
        assert hasattr(_lib.lib, name), name
        assert _lib._SIG[name] == (res, args), name
        m = re.search(rf"\b{ret}\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in ocs.h as returning {ret}"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    assert re.search(r"#define\s+OCS_LAYOUT_BATCH_MINOR\s+0\b", src) and re.search(r"#define\s+OCS_LAYOUT_TILED\s+1\b", src)


def test_layout_setting_is_host_state(pkg):
    g = pkg.RK4Integrator(np.linspace(0.0, 1.0, 9))
    assert g.layout == "batch_minor"
    assert g.set_layout("tiled").layout == "tiled"
    assert g.set_layout("batch_minor").layout == "batch_minor"
    from ocs_amd import _lib
    assert _lib.lib.ocs_integrator_set_layout(g._h, 2) == -1 and b"layout" in _lib.lib.ocs_last_error()
    assert pkg.tiled_doubles(5, 9, 17) == 2 * 16 * 45
    with pytest.raises(_lib.OcsError):   # a size is never an error code
        pkg.tiled_doubles(0, 9, 17)
