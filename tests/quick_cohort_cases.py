"""Inputs shared by test_quick_cohorts_host.py and test_gpu_quick_cohorts.py: C = 3 maps on the small grid of
tests/test_gpu_onthefly.py (its genome, region_params and sequence model; own rates, flags and gene model per cohort), a bed12 of
about 40 elements and one annotated mutation file per cohort.  No test in here."""
import numpy as np
import pandas as pd

ALL_COSMIC = ["KRAS"]
HYPER_LIMIT = 75                      # max_muts_per_sample of the cases: cohort 1 holds one sample with 90 mutations in elements, the
                                      # others about 35 each


def bed12_line(chrom, start, name, strand, blocks):
    """blocks: (offset, size) pairs from `start`."""
    end = start + blocks[-1][0] + blocks[-1][1]
    return "%s\t%d\t%d\t%s\t0\t%s\t%d\t%d\t.\t%d\t%s,\t%s,\n" % (chrom, start, end, name, strand, start, start, len(blocks),
                                                                   ",".join(str(z) for _, z in blocks), ",".join(str(o) for o, _ in blocks))


def elements(rng, window, nbins):
    """About 40 elements of 1 to 4 blocks on both strands: (name, chrom, strand, [(start, end)]); the first ones sit on window
    edges -- a block that ends exactly on one, a block across one, blocks in three windows, an element at base 0."""
    specs = [("1", 0, [(0, 300)], "+"), ("1", 2000, [(0, 1000)], "-"), ("1", 2900, [(0, 250)], "+"),
             ("2", 5100, [(0, 200), (700, 150), (1900, 400)], "-"), ("2", 9990, [(0, 5), (8, 40)], "+"), ("1", 38000, [(0, 1999)], "-")]
    for _ in range(34):
        c = "12"[int(rng.integers(0, 2))]
        st = int(rng.integers(0, nbins[c] * window - 6000))
        blocks, off = [], 0
        for _b in range(int(rng.integers(1, 5))):
            z = int(rng.integers(50, 900))
            blocks.append((off, z))
            off += z + int(rng.integers(10, 600))
        specs.append((c, st, blocks, "+-"[int(rng.integers(0, 2))]))
    lines, elts = [], []
    for i, (c, st, blocks, strand) in enumerate(specs):
        lines.append(bed12_line(c, st, "Q%02d" % i, strand, blocks))
        elts.append(("Q%02d" % i, c, strand, [(st + o, st + o + z) for o, z in blocks]))
    return "".join(lines), elts


def cohort_mutations(rng, c, elts, genes):
    """Rows of cohort c: SNVs and (not in cohort 2) indels inside the elements, background rows, exact duplicates, coding rows with
    gene labels (the expectation scaling counts them), and in cohort 1 a sample with 90 SNVs inside elements and synonymous rows
    of its own."""
    samples = ["S%d_%d" % (c, j) for j in range(9)]
    pick = lambda: samples[int(rng.integers(0, len(samples)))]
    rows = []
    for name, ch, strand, blocks in elts:
        for _ in range(int(rng.poisson(3 + c))):
            s, e = blocks[int(rng.integers(0, len(blocks)))]
            p = int(rng.integers(s, e))
            rows.append((ch, p, p + 1, "A", "T", pick(), ".", "Noncoding", "A>T", "CAG"))
        if c != 2 and rng.uniform() < 0.5:
            p = blocks[0][0]
            rows.append((ch, p, p + 2, "AG", "A", pick(), ".", "INDEL", "DEL", "."))
    for _ in range(60):
        ch = "12"[int(rng.integers(0, 2))]
        p = int(rng.integers(0, 20000))
        rows.append((ch, p, p + 1, "C", "G", pick(), ".", "Noncoding", "C>G", "ACA"))
    rows += rows[:5]
    annots = ["Synonymous", "Missense", "Nonsense", "Essential_Splice"] + (["INDEL"] if c != 2 else [])
    for _ in range(120):
        ch = "12"[int(rng.integers(0, 2))]
        p = int(rng.integers(0, 24000))
        annot = annots[int(rng.integers(0, len(annots)))]
        gene = genes[int(rng.integers(0, len(genes)))]
        if annot == "INDEL":
            rows.append((ch, p, p + 3, "ACG", "A", pick(), gene, annot, "DEL", "."))
        else:
            rows.append((ch, p, p + 1, "G", "A", pick(), gene, annot, "G>A", "AGA"))
    if c == 1:
        for i in range(90):
            name, ch, strand, blocks = elts[i % len(elts)]
            s, e = blocks[0]
            rows.append((ch, s + i % (e - s), s + i % (e - s) + 1, "T", "C", "HYPER", ".", "Noncoding", "T>C", "ATA"))
        for i in range(25):
            rows.append(("1", 30000 + i, 30001 + i, "G", "A", "HYPER", genes[i % 5], "Synonymous", "G>A", "AGA"))
    return rows


def make_case(tmp_path, seed=41):
    from digdriver_amd.io import mapfile
    from gene_cohort_cases import GENES, model_frame
    from test_gpu_onthefly import _make_case
    rng = np.random.default_rng(seed)
    base = _make_case(tmp_path, rng)
    window = base["window"]
    text, elts = elements(rng, window, {"1": 40, "2": 25})
    bed = tmp_path / "quick_elts.bed"
    bed.write_text(text)
    pres, muts = [], []
    for c in range(3):
        rp = base["rp"].copy()
        rp["Y_PRED"] = rng.gamma(9.0, 3.0, len(rp))
        rp["STD"] = rng.gamma(4.0, 1.0, len(rp))
        rp["Y_TRUE"] = rng.poisson(rp.Y_PRED.values)
        rp["FLAG"] = rng.uniform(size=len(rp)) < 0.2
        sm = base["sm"].copy()
        sm["FREQ"] = rng.dirichlet(np.ones(192)) * 1e-3
        pre = str(tmp_path / ("quick%d.map" % c))
        mapfile.write_frame(pre, "region_params", rp)
        mapfile.write_frame(pre, "sequence_model_192", sm)
        mapfile.write_frame(pre, "genic_model", model_frame(c))
        mapfile.write_array(pre, "idx", rp[["CHROM", "START", "END"]].values.astype(np.int32))
        mapfile.write_attrs(pre, cohort_name="q%d" % c, mappability_threshold=0.5)
        f = tmp_path / ("quick_muts%d.tsv" % c)
        pd.DataFrame(cohort_mutations(rng, c, elts, GENES)).to_csv(f, sep="\t", header=False, index=False)
        pres.append(pre)
        muts.append(str(f))
    return dict(maps=pres, muts=muts, fa=base["fa"], bed=str(bed), elts=elts, window=window)
