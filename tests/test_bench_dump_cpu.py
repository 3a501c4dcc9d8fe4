"""bench.py --dump-outputs: the Q1 group rows are written as float64
.npy files, the integer aggregates recoverable exactly from the 32-bit
limb array (the 128-bit decimal sums do not fit a double)."""
import numpy as np

import bench


GROUPS = [
    {"returnflag": "A", "linestatus": "F", "count": 5, "sum_qty_c": 12345,
     "sum_base_c": (1 << 62) + 1, "sum_dcol_c": 3,
     "sum_disc4": (1 << 100) + 12345, "sum_charge6": -(1 << 70) - 1},
    {"returnflag": "R", "linestatus": "O", "count": 1, "sum_qty_c": -7,
     "sum_base_c": 0, "sum_dcol_c": -1,
     "sum_disc4": (1 << 127) - 1, "sum_charge6": -(1 << 127)},
]


def test_dump_q1_outputs_exact(tmp_path):
    out = tmp_path / "dump"
    bench.dump_q1_outputs(str(out), GROUPS)
    vals = np.load(out / "q1_groups.npy")
    limbs = np.load(out / "q1_groups_limbs32.npy")
    assert vals.dtype == np.float64 and limbs.dtype == np.float64
    assert vals.shape == (2, len(bench.Q1_DUMP_COLS))
    assert limbs.shape == (2, len(bench.Q1_DUMP_COLS) - 2, 4)
    for i, g in enumerate(GROUPS):
        assert vals[i, 0] == ord(g["returnflag"])
        assert vals[i, 1] == ord(g["linestatus"])
        for j, key in enumerate(bench.Q1_DUMP_COLS[2:]):
            assert vals[i, 2 + j] == float(g[key])
            u = sum(int(limbs[i, j, k]) << (32 * k) for k in range(4))
            if u >= 1 << 127:
                u -= 1 << 128
            assert u == g[key], (i, key)


def test_dump_q1_outputs_deterministic(tmp_path):
    bench.dump_q1_outputs(str(tmp_path / "a"), GROUPS)
    bench.dump_q1_outputs(str(tmp_path / "b"), GROUPS)
    for name in ("q1_groups.npy", "q1_groups_limbs32.npy"):
        assert (tmp_path / "a" / name).read_bytes() == \
            (tmp_path / "b" / name).read_bytes()
