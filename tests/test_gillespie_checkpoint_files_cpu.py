"""CPU suite: the .npz files of gillespie.Checkpoint and gillespie.MixedCheckpoint, member for member.

tests/golden/checkpoint_plain.npz, checkpoint_mixed.npz and checkpoint_mixed_structure.npz were saved by `Checkpoint.save` and
`MixedCheckpoint.save` of commit 5dbba22 from the checkpoints `golden_checkpoints` builds (S = 3, n_cap = 7, L = 50: the
`make_checkpoint` of tests/test_gillespie_mixed_resume_cpu.py), by this file's own

    python tests/test_gillespie_checkpoint_files_cpu.py --record      (run in a checkout of the commit to record from)

Each file must load with the code as it is now into what the constructor was given, and saving it again must give the same
members: their names, every member's dtype, shape and bytes, and the parsed `meta`.  (The .npz bytes themselves are not
compared: a zip archive carries the time it was written.)"""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gillespie_mixed_resume_cpu import PKG, make_checkpoint    # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
gil = importlib.import_module(PKG + ".gillespie")
PLAIN = dict(local_kernel_sigma=0.03, seed=7, streams="batch")       # what a Checkpoint has and `make_checkpoint` does not give
MIXED_FIELDS = ("pos", "flags", "ref", "t", "n_events", "next_obs", "n_slots", "seeds", "streams", "sigma_grids", "L", "K", "periodic", "anchor_mask",
                "obs_dt", "large", "block_tables", "k_max", "first_obs", "window", "n_window", "n_empty")
PLAIN_FIELDS = ("pos", "flags", "ref", "t", "n_events", "next_obs", "L", "K", "periodic", "local_kernel_sigma", "anchor_mask", "seed", "streams", "obs_dt")


def golden_checkpoints():
    """name -> (class, fields to compare, the checkpoint as the constructor makes it)"""
    mixed, structure = make_checkpoint(gil), make_checkpoint(gil, structure=True, block_tables=None)
    plain = gil.Checkpoint(**{k: getattr(mixed, k) for k in PLAIN_FIELDS if k not in PLAIN}, **PLAIN)
    return {"checkpoint_plain": (gil.Checkpoint, PLAIN_FIELDS, plain), "checkpoint_mixed": (gil.MixedCheckpoint, MIXED_FIELDS, mixed),
            "checkpoint_mixed_structure": (gil.MixedCheckpoint, MIXED_FIELDS, structure)}


def members(path):
    with np.load(path, allow_pickle=False) as z:
        out = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files if k != "meta"}
        return out, json.loads(str(z["meta"]))


@pytest.mark.parametrize("name", sorted(golden_checkpoints()))
def test_a_recorded_file_loads_into_the_constructor_inputs_and_saves_into_the_same_members(name, tmp_path):
    cls, fields, made = golden_checkpoints()[name]
    back = cls.load(os.path.join(GOLDEN, name + ".npz"))
    assert type(back) is cls
    for k in fields:
        a, b = getattr(made, k), getattr(back, k)
        if isinstance(a, np.ndarray):
            assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        else:
            assert type(a) is type(b) and a == b, k
    again = tmp_path / "again.npz"
    back.save(again)
    got, want = members(again), members(os.path.join(GOLDEN, name + ".npz"))
    assert sorted(got[0]) == sorted(want[0])
    for k in want[0]:
        assert got[0][k] == want[0][k], k
    assert got[1] == want[1]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gillespie_checkpoint_files_cpu.py --record   (in a checkout of the commit to record from)")
    for name, (_, _, made) in golden_checkpoints().items():
        made.save(os.path.join(GOLDEN, name + ".npz"))
        print(name, os.path.getsize(os.path.join(GOLDEN, name + ".npz")), "bytes")
