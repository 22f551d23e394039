"""h5lite.append_dataset: a new root-level dataset in an existing HDF5 file without reading or rewriting what is in it -- on files
the HDF5 library wrote (a committed one, and fresh ones from h5py where the image has its second interpreter), checked byte for byte
below the old end of file and read back by h5lite and by h5py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from digdriver_amd.io import h5lite, mapfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENUINE = os.path.join(ROOT, "tests", "golden", "element_data_genuine.h5")
PY39 = "/opt/conda/bin/python3.9"


def _patched(path):
    """The byte ranges append_dataset may change below the old end of file: the superblock's end-of-file address and root entry
    scratch, and the (B-tree, heap) addresses of the root object header's symbol-table message."""
    buf = open(path, "rb").read()
    assert buf[:8] == h5lite.SIG and buf[8] == 0                    # superblock version 0 at offset 0
    hdr = int.from_bytes(buf[64:72], "little")                      # the root entry's object header address
    assert buf[hdr] == 1
    u = lambda off, n: int.from_bytes(buf[off:off + n], "little")
    blocks, at = [(hdr + 16, hdr + 16 + u(hdr + 8, 4))], None
    while blocks:                                                   # (the library moves messages to continuation blocks)
        q, hi = blocks.pop(0)
        while q + 8 <= hi:
            mtype, msize = u(q, 2), u(q + 2, 2)
            if mtype == 0x11:
                at = q + 8
            elif mtype == 0x10:
                blocks.append((u(q + 8, 8), u(q + 8, 8) + u(q + 16, 8)))
            q += 8 + msize
    assert at is not None
    return [(40, 48), (80, 96), (at, at + 16)]


def _assert_only_patched(before, path, ranges):
    after = open(path, "rb").read()
    assert len(after) > len(before)
    diff = np.flatnonzero(np.frombuffer(before, np.uint8) != np.frombuffer(after[:len(before)], np.uint8))
    assert len(diff) > 0
    for i in diff.tolist():
        assert any(lo <= i < hi for lo, hi in ranges), "byte %d below the old end of file changed" % i


def test_append_to_a_file_the_hdf5_library_wrote(tmp_path):
    p = str(tmp_path / "data.h5")
    shutil.copy(GENUINE, p)
    old = h5lite.read_tree(p)
    old_keys = list(old.keys())
    ranges = _patched(p)
    before = open(p, "rb").read()
    lab = np.arange(7, dtype=np.float64) * 1.5
    h5lite.append_dataset(p, "Cohort_A", lab)
    _assert_only_patched(before, p, ranges)
    new = h5lite.read_tree(p)
    assert sorted(new.keys()) == sorted(old_keys + ["Cohort_A"])
    assert new["Cohort_A"].data.dtype == np.float64 and np.array_equal(new["Cohort_A"].data, lab)
    assert np.array_equal(new["substitution_idx"].data, old["substitution_idx"].data)
    # more names than one symbol-table node holds (2 * 4 entries): the node splits, the B-tree gets a second leaf
    for i in range(12):
        h5lite.append_dataset(p, "L%02d" % i, np.full(3, i, np.int32))
    _assert_only_patched(before, p, ranges)
    new = h5lite.read_tree(p)
    assert sorted(new.keys()) == sorted(old_keys + ["Cohort_A"] + ["L%02d" % i for i in range(12)])
    assert all(np.array_equal(new["L%02d" % i].data, np.full(3, i, np.int32)) for i in range(12))
    assert np.array_equal(new["Cohort_A"].data, lab)
    with pytest.raises(h5lite.H5LiteError, match="name already exists"):
        h5lite.append_dataset(p, "L03", np.zeros(2))
    with pytest.raises(h5lite.H5LiteError, match="plain name"):
        h5lite.append_dataset(p, "grp/x", np.zeros(2))


def test_append_to_a_file_h5lite_wrote_and_through_mapfile(tmp_path):
    p = str(tmp_path / "ours.h5")
    mapfile.write_array(p, "idx", np.array([[1, 0, 10], [2, 0, 10]], np.int32))
    mapfile.write_attrs(p, cohort_name="X")
    ranges, before = _patched(p), open(p, "rb").read()
    mapfile.write_array(p, "Cohort_B", np.array([3.0, 4.0]), append=True)
    _assert_only_patched(before, p, ranges)
    assert np.array_equal(mapfile.read_array(p, "Cohort_B"), [3.0, 4.0]) and mapfile.read_attrs(p)["cohort_name"] == "X"
    assert np.array_equal(mapfile.read_array(p, "idx"), [[1, 0, 10], [2, 0, 10]])
    with pytest.raises(mapfile.MapFileError, match="name already exists"):
        mapfile.write_array(p, "Cohort_B", np.zeros(2), append=True)
    mapfile.write_array(p, "Cohort_B", np.zeros(2))                  # (without append: replaced, the file rewritten)
    assert np.array_equal(mapfile.read_array(p, "Cohort_B"), [0.0, 0.0])
    # a map that does not exist yet, and the directory mirror, take append=True as a plain write
    q = str(tmp_path / "new.h5")
    mapfile.write_array(q, "a", np.arange(3), append=True)
    assert np.array_equal(mapfile.read_array(q, "a"), [0, 1, 2])
    d = str(tmp_path / "mirror")
    mapfile.write_array(d, "a", np.arange(3), append=True)
    assert np.array_equal(mapfile.read_array(d, "a"), [0, 1, 2])


_H5PY_CHILD = r"""
import json, sys
import h5py, numpy as np
mode, path = sys.argv[1], sys.argv[2]
if mode == "write":
    rng = np.random.default_rng(3)
    with h5py.File(path, "w") as f:
        f.create_dataset("idx", data=np.stack([np.ones(50, np.int32), np.arange(50, dtype=np.int32) * 100, np.arange(1, 51, dtype=np.int32) * 100], 1))
        f.create_dataset("x_data", data=rng.integers(0, 100, (50, 20, 4)).astype(np.float32), chunks=(5, 20, 4), compression="gzip")
        f.create_dataset("mappability", data=rng.uniform(size=50).astype(np.float32))
        f.create_group("meta").create_dataset("tracks", data=np.arange(4))
        f.attrs["note"] = "written by h5py"
    with h5py.File(path, "r") as f:
        np.savez(path + ".npz", idx=f["idx"][:], x=f["x_data"][:], mapp=f["mappability"][:])
elif mode == "write_latest":
    with h5py.File(path, "w", libver="latest") as f:
        f.create_dataset("idx", data=np.zeros((2, 3), np.int32))
else:
    with h5py.File(path, "r") as f:
        out = {"keys": sorted(f.keys()), "note": f.attrs["note"], "tracks": f["meta/tracks"][:].tolist()}
        out["labels"] = {k: f[k][:].tolist() for k in f.keys() if k.startswith(("Cohort", "L"))}
        out["dtype"] = str(f["Cohort_A"].dtype)
        out["x_sum"] = float(f["x_data"][:].sum())
        out["idx0"] = f["idx"][:2].tolist()
    with h5py.File(path, "r+") as f:                                  # the library can go on extending the group
        f.create_dataset("later", data=[1, 2, 3])
    with h5py.File(path, "r") as f:
        out["later"] = f["later"][:].tolist()
        out["n"] = len(f.keys())
    print(json.dumps(out))
"""


@pytest.mark.skipif(not os.path.exists(PY39), reason="LOUD SKIP: %s (the interpreter with h5py) is not in this image -- the "
                    "cross-check of append_dataset against the HDF5 library cannot run here" % PY39)
def test_append_cross_checked_with_h5py(tmp_path):
    probe = subprocess.run([PY39, "-c", "import h5py"], capture_output=True)
    if probe.returncode != 0:
        pytest.skip("LOUD SKIP: h5py does not import under %s" % PY39)
    child = tmp_path / "child.py"
    child.write_text(_H5PY_CHILD)
    p = str(tmp_path / "train.h5")
    r = subprocess.run([PY39, str(child), "write", p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = np.load(p + ".npz")
    ranges = _patched(p)
    before = open(p, "rb").read()
    labels = {"Cohort_A": np.arange(50, dtype=np.float64)}
    labels.update({"L%02d" % i: np.full(50, i + 0.5) for i in range(10)})          # 4 + 11 names: one node (8) cannot hold them
    for k, v in labels.items():
        mapfile.write_array(p, k, v, append=True)
    _assert_only_patched(before, p, ranges)
    for k, v in labels.items():
        assert np.array_equal(mapfile.read_array(p, k), v)
    assert np.array_equal(mapfile.read_array(p, "x_data"), want["x"]) and np.array_equal(mapfile.read_array(p, "idx"), want["idx"])
    r = subprocess.run([PY39, str(child), "read", p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().split("\n")[-1])
    assert got["keys"] == sorted(["idx", "x_data", "mappability", "meta"] + list(labels))
    assert got["note"] == "written by h5py" and got["tracks"] == [0, 1, 2, 3] and got["dtype"] == "float64"
    assert got["labels"] == {k: v.tolist() for k, v in labels.items()}
    assert got["x_sum"] == float(want["x"].sum()) and got["idx0"] == want["idx"][:2].tolist()
    assert got["later"] == [1, 2, 3] and got["n"] == 4 + len(labels) + 1
    # a root group of the new format is refused, and the message names the feature
    q = str(tmp_path / "latest.h5")
    r = subprocess.run([PY39, str(child), "write_latest", q], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    before = open(q, "rb").read()
    with pytest.raises(h5lite.H5LiteError, match="new-style root group"):
        h5lite.append_dataset(q, "Cohort_A", np.zeros(2))
    assert open(q, "rb").read() == before
