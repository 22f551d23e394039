"""Generate the copy-number training-label golden (DataExtractor addObjectives --cnv) by running the REAL reference's
fetch_cnv_region_avg here.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference):

    python tests/golden/make_cnv_golden.py

* Stubs the reference's absent I/O-only dependencies as make_objectives_golden.py does and imports scripts/DataExtractor.py of the
  reference from its own location; no bytecode is written.
* The reference reads its segments through pysam.TabixFile.fetch.  It is handed a stub whose fetch(reference, start, end) returns, as
  text rows in file order, the rows of the cohort whose chromosome label equals `reference` and that satisfy the overlap rule of a
  bed-preset index: row start < end and row end > start (0-based, half-open).  Everything behind the fetch is the reference's own code;
  the loop over the windows restates DataExtractor.py:530,538-539 (add_objectives itself opens an h5py file).  A window without a row
  comes back as the all-zero [W, 3] track (fetch_cnv_region_avg returns the track itself there): stored as [0, 0, 0].
* Inputs: 60 windows of W = 100 on chromosomes 1 (tiling from 1 000), 2 (stride 150: gaps; listed in descending order) and 7 (tiling
  from 0), and three cohorts: `mixed` (the hand-made cases below and seeded random segments), `sparse` (a few segments: most windows see
  none) and `none` (no row at all).  Hand-made: a segment over a whole chromosome; one inside a single window; one that ends exactly at a
  window's end; one that ends exactly at a window's start and one that starts exactly at a window's end (neither overlaps it); one that
  starts before the first window; one of a single base; cp_num 0, 1, 2, 3 and 8, a "3.0"; cp_num 2 with cp_min 0 and with cp_min 1 (both
  LOH); duplicate rows; rows on chromosome 3 and on 'chr1', which idx does not hold.
* Stores inputs and expected labels in cnv_objectives_golden.json.gz -- data only.
"""
import gzip
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cnv_objectives_golden.json.gz")
W = 100


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, REF)


def reference_module():
    spec = importlib.util.spec_from_file_location("reference_data_extractor", os.path.join(REF, "scripts", "DataExtractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class StubTabix:
    """What pysam.TabixFile answers for a bed-preset index over `rows` (lists of seven text fields)."""

    def __init__(self, rows):
        self.rows = rows

    def fetch(self, reference=None, start=None, end=None):
        return ["\t".join(r) for r in self.rows if r[0] == reference and int(r[1]) < end and int(r[2]) > start]


def windows():
    idx = [(1, 1_000 + W * i, 1_000 + W * (i + 1)) for i in range(20)]
    idx += [(2, 500 + 150 * i, 500 + 150 * i + W) for i in range(20)][::-1]
    idx += [(7, W * i, W * (i + 1)) for i in range(20)]
    return idx


def cohorts(rng):
    def seg(ch, start, end, cp, cp_min=None, donor="D0"):
        cp_min = min(int(float(cp)), 1) if cp_min is None else cp_min
        return [str(ch), str(int(start)), str(int(end)), str(cp), str(max(int(float(cp)) - cp_min, 0)), str(cp_min), donor]

    mixed = [
        seg(7, 0, 2_000, 3),                         # a whole chromosome's windows
        seg(1, 0, 10_000, 1, donor="D1"),            # the same, starting before the first window and ending behind the last
        seg(1, 1_210, 1_260, 8),                     # inside a single window
        seg(1, 1_300, 1_500, 0),                     # from a window's start exactly to a window's end
        seg(1, 1_450, 1_600, 3),                     # ends exactly at a window's end = the next one's start: no overlap with that one
        seg(1, 1_700, 1_800, "3.0"),                 # exactly one window
        seg(1, 2_999, 3_000, 1),                     # the last base of the last window
        seg(1, 3_000, 3_100, 1),                     # starts exactly at the last window's end: no overlap
        seg(1, 900, 1_000, 8),                       # ends exactly at the first window's start: no overlap
        seg(1, 950, 1_001, 2, cp_min=0),             # starts before the first window, one base of it; LOH with cp_min 0
        seg(1, 1_050, 1_950, 2, cp_min=1),           # cp_num 2 counts as LOH whatever cp_min says
        seg(2, 560, 640, 0),                         # across chromosome 2's first window's end into the gap
        seg(2, 610, 640, 8),                         # inside a gap: no window
        seg(2, 590, 1_420, 3),                       # partial, whole windows with gaps between, partial
        seg(7, 5, 6, 0),                             # one base
        seg(7, 1_999, 2_500, 1),                     # the last base of the last window and beyond
        seg(3, 0, 5_000, 8), seg("chr1", 1_000, 3_000, 8),          # chromosomes idx does not hold
    ]
    mixed += [list(mixed[2]), list(mixed[2]), list(mixed[13])]      # duplicate rows count again
    for _ in range(50):
        ch = (1, 2, 7)[rng.integers(3)]
        lo = {1: 900, 2: 400, 7: 0}[ch]
        start = int(lo + rng.integers(0, 2_300))
        length = int([rng.integers(1, 40), rng.integers(40, 400), rng.integers(400, 3_000)][rng.integers(3)])
        mixed.append(seg(ch, start, start + length, (0, 1, 2, 3, 8, 4)[rng.integers(6)], donor="D%d" % rng.integers(5)))
    sparse = [seg(1, 1_850, 1_905, 3), seg(7, 300, 700, 1), seg(7, 650, 651, 2), seg(2, 3_350, 3_351, 8)]
    return {"mixed": mixed, "sparse": sparse, "none": []}


def reference_labels(ref, idx, rows):
    tbx = StubTabix(rows)
    window = idx[0][2] - idx[0][1]
    out = []
    for w in idx:
        avg = np.asarray(ref.fetch_cnv_region_avg(tbx, str(w[0]), w[1], window))
        if avg.shape != (3,):
            assert avg.shape == (window, 3) and not avg.any()
            avg = np.zeros(3)
        out.append([float(x) for x in avg])
    return out


def main():
    install_stubs()
    ref = reference_module()
    rng = np.random.default_rng(20261020)
    idx = windows()
    rows = cohorts(rng)
    labels = {name: reference_labels(ref, idx, r) for name, r in rows.items()}
    mixed, sparse = np.array(labels["mixed"]), np.array(labels["sparse"])
    assert not np.array(labels["none"]).any()
    assert (mixed.sum(axis=0) > 0).all()                                                        # every class occurs
    assert (sparse.sum(axis=1) == 0).sum() > 40 and sparse.sum() > 0                           # most windows see no segment
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(dict(W=W, idx=[list(w) for w in idx], cohorts=rows, labels=labels), separators=(",", ":")).encode())
    print("wrote %s (%d bytes): %d windows, cohorts of %s rows" % (OUT, os.path.getsize(OUT), len(idx), [len(v) for v in rows.values()]))


if __name__ == "__main__":
    main()
