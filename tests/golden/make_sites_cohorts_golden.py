"""Generate the many-cohort sites golden (elementDriver --f-sites for C cohorts) by running the REAL reference per cohort here.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference):

    python tests/golden/make_sites_cohorts_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does and imports the reference from its own location; no
  bytecode is written.
* Per (cohort, element frame) the reference's own tabulate_sites_in_element, transfer_element_model, element_expected_muts_nb,
  element_pvalue_burden_nb and element_pvalue_burden_nb_by_sample run on a synthetic element frame (the columns load_pretrained_model
  leaves: R_OBS, MU, SIGMA, ALPHA, THETA, Pi_SUM) with a given scale factor: run_sites_region_model (transfer_tools.py:1098-1169)
  behind its map reading and scale-factor rules.  None of them needs bedtools.
* Inputs.  One sites file, 10 columns with the element in the SAMPLE column, about 40 rows over the 6 elements A B C D E X: a position
  listed by two elements (A and B), a whole row listed twice in C, two sites of A that differ only in ALT, two of B only in END, two of
  D only in GENE, a row of E whose CONTEXT field is `nan`, a row without an element label, and a site on chromosome X.  Two element
  frames: `full` = A B C D E Z (X is an element the model lacks, Z a model element no site names) and `hit` = A B C D E.  Three cohorts:
  `hits` (exact hits; one near miss in each of the nine columns; a missing-CONTEXT row at the `nan` site; duplicate rows; a row that
  hits the position two elements list and the row listed twice; an INDEL at a site position; rows on X; Synonymous rows with and without
  TP53), `none` (near misses, X rows and an INDEL only: no hit at all) and `all` (every element of `hit` is hit: with that frame the
  OBS columns stay int64).  For `none` the reference's own by-sample p-value step fails -- its empty count table has an object
  OBS_SAMPLES column, which scipy refuses -- so that cohort's frames end at PVAL_SNV_BURDEN and say so (`pvalues_failed`); its
  counts, all zero, are the reference's.
* Stores inputs, the count tables and the frames in sites_cohorts_golden.json -- data only.
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import pandas as pd

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sites_cohorts_golden.json")
BASES = "ACGT"
SCALE = {"hits": 0.8, "none": 1.7, "all": 0.05}


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, REF)


def make_sites(rng):
    """Site rows [CHROM, START, END, REF, ALT, ELT, GENE, ANNOT, MUT_TYPE, CONTEXT] and the places of the special ones."""
    def site(elt, ch, pos, gene, annot="Noncoding"):
        ref = BASES[rng.integers(4)]
        alt = BASES[(BASES.index(ref) + 1 + rng.integers(3)) % 4]
        ctx = BASES[rng.integers(4)] + ref + BASES[rng.integers(4)]
        return [str(ch), int(pos), int(pos) + 1, ref, alt, elt, gene, annot, ref + ">" + alt, ctx]

    rows, special = [], {}
    for k, elt in enumerate("ABCDEX"):
        for q in range(5):
            rows.append(site(elt, 1 + (k + q) % 3, 1000 * (k + 1) + 37 * q, "G" + elt, "Missense" if q % 2 else "Noncoding"))
    special["plain"] = {elt: 5 * k for k, elt in enumerate("ABCDEX")}            # a plain site of every element
    a = site("A", 2, 50000, "GA")
    special["shared"] = len(rows)
    rows += [a, a[:5] + ["B"] + a[6:]]                                            # one position, two elements
    c = site("C", 3, 51000, "GC")
    special["twice"] = len(rows)
    rows += [c, list(c)]                                                          # a whole row twice in one element
    a = site("A", 1, 52000, "GA")
    other = [b for b in BASES if b not in (a[3], a[4])][0]
    special["alt"] = len(rows)
    rows += [a, a[:4] + [other] + a[5:]]                                          # differ only in ALT (MUT_TYPE kept)
    b = site("B", 2, 53000, "GB")
    special["end"] = len(rows)
    rows += [b, b[:2] + [b[2] + 1] + b[3:]]                                       # differ only in END
    d = site("D", 3, 54000, "GD")
    special["gene"] = len(rows)
    rows += [d, d[:6] + ["GD2"] + d[7:]]                                          # differ only in GENE
    e = site("E", 1, 55000, "GE")
    special["nan"] = len(rows)
    rows.append(e[:9] + ["nan"])                                                  # a CONTEXT pandas reads as missing
    special["unnamed"] = len(rows)
    rows.append(site("", 2, 56000, "GN"))                                         # no element label
    special["sex"] = len(rows)
    rows.append(site("D", "X", 57000, "GD"))
    return rows, special


def make_cohorts(rng, sites, special):
    def hit(i, samp):
        s = sites[i]
        return s[:5] + [samp] + s[6:]

    def misses(i, samp):
        """one near miss of site i in each of the nine columns"""
        s, out = hit(i, samp), []
        for col in (0, 1, 2, 3, 4, 6, 7, 8, 9):
            r = list(s)
            if col == 0:
                r[0] = str(int(s[0]) % 22 + 1)
            elif col in (1, 2):
                r[col] = s[col] + 1
            elif col in (3, 4):
                r[col] = [b for b in BASES if b not in (s[3], s[4])][0]
            elif col == 9:
                r[9] = s[9][0] + s[9][1] + BASES[(BASES.index(s[9][2]) + 1) % 4]
            else:
                r[col] = s[col] + "_"
            out.append(r)
        return out

    def background(n, annot, gene):
        out = []
        for _ in range(n):
            ref = BASES[rng.integers(4)]
            alt = BASES[(BASES.index(ref) + 1) % 4]
            out.append([str(int(rng.integers(1, 23))), int(rng.integers(10 ** 5, 10 ** 6)), 0, ref, alt, "S%d" % rng.integers(6), gene,
                        annot, ref + ">" + alt, "A" + ref + "C"])
            out[-1][2] = out[-1][1] + 1
        return out

    p = special["plain"]
    x_rows = [hit(special["sex"], "S1"), hit(special["sex"], "S2")]
    indel = lambda i, samp: hit(i, samp)[:7] + ["INDEL"] + hit(i, samp)[8:]
    hits = [hit(p["A"], "S0"), hit(p["A"], "S1"), hit(p["A"], "S1"),             # a duplicate row: counts twice, one sample
            hit(p["B"] + 1, "S2"), hit(p["D"] + 2, "S0"), hit(p["X"], "S3"), hit(p["X"] + 1, "S3"),
            hit(special["shared"], "S4"),                                         # counts for A and for B
            hit(special["twice"], "S5"), hit(special["twice"], "S0"),             # each counts twice for C
            hit(special["alt"], "S1"), hit(special["alt"] + 1, "S2"),
            hit(special["end"] + 1, "S3"),
            hit(special["gene"], "S4"), hit(special["gene"] + 1, "S4"),
            hit(special["nan"], "S5")[:9] + [""],                                 # a missing CONTEXT at the `nan` site
            hit(special["nan"], "S0")[:9] + ["NA"],
            hit(special["unnamed"], "S1"),                                        # the site without an element: counted nowhere
            indel(p["A"], "S2")]
    hits += misses(p["A"], "S3") + misses(special["gene"], "S1") + x_rows
    hits += background(7, "Synonymous", "GSYN") + background(2, "Synonymous", "TP53") + background(5, "Missense", "GMIS")
    none = misses(p["B"], "T0") + misses(p["E"] + 3, "T1") + x_rows + [indel(p["C"], "T2")] + background(4, "Synonymous", "GSYN")
    every = [hit(p[elt] + q, "U%d" % ((k + q) % 3)) for k, elt in enumerate("ABCDE") for q in range(2)]
    every += [hit(p["A"], "U0"), hit(special["twice"], "U2")] + background(3, "Synonymous", "GSYN")
    text = lambda rows: "".join("\t".join(str(v) for v in r) + "\n" for r in rows)
    return dict(hits=text(hits), none=text(none), all=text(every))


def element_frame(rng, names, nb):
    mu, sigma = rng.gamma(4.0, 0.05, len(names)), rng.gamma(4.0, 0.02, len(names))
    alpha, theta = nb.normal_params_to_gamma(mu, sigma)
    frame = pd.DataFrame({"R_OBS": rng.integers(0, 40, len(names)), "MU": mu, "SIGMA": sigma, "ALPHA": alpha, "THETA": theta,
                          "Pi_SUM": rng.uniform(0.05, 0.6, len(names))}, index=pd.Index(names, name="ELT"))
    return frame


def main():
    install_stubs()
    from DIGDriver.data_tools import mutation_tools as ref_mt           # noqa: E402
    from DIGDriver.driver_model import transfer_tools as ref_tt         # noqa: E402
    from DIGDriver.sequence_model import nb_model as ref_nb             # noqa: E402

    rng = np.random.default_rng(20261019)
    sites, special = make_sites(rng)
    cohorts = make_cohorts(rng, sites, special)
    sites_text = "".join("\t".join(str(v) for v in r) + "\n" for r in sites)
    models = {"full": element_frame(rng, list("ABCDEZ"), ref_nb), "hit": element_frame(rng, list("ABCDE"), ref_nb)}
    out = dict(sites=sites_text, special=special, cohorts=cohorts, scale=SCALE, tables={}, frames=[],
               models={k: dict(index=list(m.index), columns={c: m[c].tolist() for c in m.columns}) for k, m in models.items()})
    with tempfile.TemporaryDirectory() as tmp:
        f_sites = os.path.join(tmp, "sites.txt")
        with open(f_sites, "w") as f:
            f.write(sites_text)
        for name, text in cohorts.items():
            f_mut = os.path.join(tmp, name + ".txt")
            with open(f_mut, "w") as f:
                f.write(text)
            table = ref_mt.tabulate_sites_in_element(f_sites, f_mut)
            out["tables"][name] = dict(index=[str(i) for i in table.index], OBS_SAMPLES=[int(v) for v in table.OBS_SAMPLES],
                                       OBS_SNV=[int(v) for v in table.OBS_SNV])
            for key, model in models.items():
                df = ref_tt.transfer_element_model(table, model.copy(), SCALE[name], use_chrom=False)
                df = ref_tt.element_expected_muts_nb(df)
                failed = None
                try:
                    df = ref_tt.element_pvalue_burden_nb_by_sample(ref_tt.element_pvalue_burden_nb(df))
                except TypeError as exc:                     # (an empty count table: object columns, which scipy refuses)
                    assert len(table) == 0
                    failed = "TypeError: " + str(exc)
                out["frames"].append(dict(cohort=name, model=key, index=list(df.index), order=list(df.columns), pvalues_failed=failed,
                                          dtypes={c: str(df[c].dtype) for c in df.columns},
                                          columns={c: [float(v) for v in df[c]] for c in df.columns}))
                print(name, key, "OBS_SNV", df.OBS_SNV.tolist(), df.OBS_SNV.dtype)
    with open(OUT, "w") as f:
        json.dump(out, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
