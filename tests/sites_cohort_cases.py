"""What the sites-of-many-cohorts tests share: the golden (tests/golden/sites_cohorts_golden.json, made by the reference's own code per
cohort), its files and maps written to a directory, the encoded arrays of a case, and -- for a machine without a card -- the stand-ins
of the library calls (the plain statement for the counting, the scipy oracle for the two element-wise statistics)."""
import json
import os

import numpy as np
import pandas as pd

import gene_cohort_cases as GK
import sites_statement as S
from conftest import GOLDEN
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools import sites
from digdriver_amd.io import mapfile
from digdriver_amd.sequence_model import nb_model

FX = json.load(open(os.path.join(GOLDEN, "sites_cohorts_golden.json")))
COHORTS = ["hits", "none", "all"]
KEY = "mysites"


def has_card():
    try:
        return _lib.device_count() > 0
    except _lib.DigHipError:
        return False                                                    # (the library has not been built)


def stand_in_without_a_card(monkeypatch):
    """Without a card the statement counts and scipy computes the Gamma parameters and the mid-p values, for the serial and the
    batched route alike (both reach them through these module attributes); everything around them is the product's either way."""
    if has_card():
        return
    from oracle import dig_oracle as O
    f64 = lambda *xs: [np.asarray(x, np.float64) for x in xs]
    monkeypatch.setattr(engine, "site_counts", S.site_counts)
    monkeypatch.setattr(nb_model, "normal_params_to_gamma", lambda mu, sigma, device=0: O.normal_params_to_gamma(*f64(mu, sigma)))
    monkeypatch.setattr(nb_model, "nb_pvalue_greater_midp", lambda k, alpha, p, device=0: O.nb_pvalue_greater_midp(*f64(k, alpha, p)))


def write_files(tmp, names=COHORTS):
    """(f_sites, [f_mut per name])"""
    f_sites = str(tmp / "sites.txt")
    with open(f_sites, "w") as f:
        f.write(FX["sites"])
    f_muts = []
    for name in names:
        f_muts.append(str(tmp / (name + ".annot.txt")))
        with open(f_muts[-1], "w") as f:
            f.write(FX["cohorts"][name])
    return f_sites, f_muts


def element_frame(which, c=0):
    """The stored element model of cohort c: the golden's frame `which` for c == 0, the same elements with other rates after it."""
    m = FX["models"][which]
    frame = pd.DataFrame({"ELT": m["index"], "R_OBS": m["columns"]["R_OBS"], "MU": m["columns"]["MU"], "SIGMA": m["columns"]["SIGMA"],
                          "P_SUM": m["columns"]["Pi_SUM"]})
    if c:
        rng = np.random.RandomState(900 + c)
        frame["MU"] = frame.MU * rng.uniform(0.5, 2.0, len(frame))
        frame["SIGMA"] = frame.SIGMA * rng.uniform(0.5, 2.0, len(frame))
    return frame


def write_maps(tmp, which, C, same_rates=False):
    """C maps with the element model `which` under KEY and a gene model of their own."""
    paths = []
    for c in range(C):
        paths.append(str(tmp / ("%s%d.map" % (which, c))))
        mapfile.write_frame(paths[-1], KEY, element_frame(which, 0 if same_rates else c))
        mapfile.write_frame(paths[-1], "genic_model", GK.model_frame(c))
    return paths


def encoded(f_sites, f_muts):
    """The arguments of engine.site_counts for the files, as host arrays: (args, element names)."""
    table = sites.encode_sites_file(f_sites)
    rows = [sites.encode_site_rows(f, table["dicts"], c) for c, f in enumerate(f_muts)]
    off = np.concatenate([[0], np.cumsum([len(r["sample_names"]) for r in rows])]).astype(np.int64)
    cat = lambda k: np.concatenate([r[k] for r in rows])
    sample = np.concatenate([r["sample"] + np.int32(off[c]) for c, r in enumerate(rows)]).astype(np.int32)
    args = (table["site_pos"], table["site_end"], table["site_attr"], table["site_elt"], cat("pos"), cat("end"), cat("attr"), sample,
            cat("cohort"), off, len(table["elt_names"]), len(f_muts))
    return args, table["elt_names"], rows


def count_table(counts, names, c):
    """The reference's count table of cohort c from [E, C] planes: element -> (OBS_SAMPLES, OBS_SNV), elements with a row only."""
    snv, samples = np.asarray(counts["obs_snv"]), np.asarray(counts["obs_samples"])
    return {n: (int(samples[e, c]), int(snv[e, c])) for e, n in enumerate(names) if snv[e, c] > 0}


def golden_table(name):
    t = FX["tables"][name]
    return {n: (a, b) for n, a, b in zip(t["index"], t["OBS_SAMPLES"], t["OBS_SNV"])}


def golden_frame(name, which):
    return [f for f in FX["frames"] if f["cohort"] == name and f["model"] == which][0]
