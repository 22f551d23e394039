"""An independent statement of the gene route's observed counts for several cohorts in plain Python: dicts and loops over
(gene, sample, annotation) tuples.

Written from the rule, not from the kernel.  A cohort's coding rows are (gene label, sample label, annotation label) tuples.
  * A sample with more than `max_muts_per_sample` rows -- rows of every gene and every annotation -- is blacklisted, and none of
    its rows counts below.
  * OBS of (gene, class), class one of Synonymous, Missense, Nonsense, Essential_Splice, INDEL: over the samples, the number of
    rows of (gene, sample, class), each clipped to `max_muts_per_gene_per_sample` as a number; the sum, cast to int.  Only genes of
    the model have an OBS.
  * N_SAMP of (gene, class), class one of SYN, MIS, NONS, SPL, TRUNC = Nonsense or Essential_Splice, NONSYN = Missense, Nonsense or
    Essential_Splice, INDEL: the number of samples with at least one row of the gene in the class.  Not clipped.
  * n_syn: the number of Synonymous rows whose gene is not TP53 -- genes outside the model included.  Not clipped.
  * pairs of a gene: the number of samples with a row of the gene of ANY annotation.
"""
OBS_CLASSES = ("Synonymous", "Missense", "Nonsense", "Essential_Splice", "INDEL")
N_SAMP_CLASSES = {"SYN": ("Synonymous",), "MIS": ("Missense",), "NONS": ("Nonsense",), "SPL": ("Essential_Splice",),
                  "TRUNC": ("Nonsense", "Essential_Splice"), "NONSYN": ("Missense", "Nonsense", "Essential_Splice"),
                  "INDEL": ("INDEL",)}


def cohort_counts(rows, genes, max_muts_per_sample, max_muts_per_gene_per_sample):
    """rows: list of (gene, sample, annot) of one cohort; genes: the model's gene labels.
    Returns dict(obs={(gene, annot): int}, n_samp={(gene, class): int}, n_syn=int, blacklist=set of samples,
    pairs={gene: int}); genes and classes without a row are absent (= 0)."""
    per_sample = {}
    for gene, sample, annot in rows:
        per_sample[sample] = per_sample.get(sample, 0) + 1
    blacklist = {s for s, n in per_sample.items() if n > max_muts_per_sample}
    in_model = set(genes)
    group = {}
    n_syn = 0
    for gene, sample, annot in rows:
        if sample in blacklist:
            continue
        group[(gene, sample, annot)] = group.get((gene, sample, annot), 0) + 1
        if annot == "Synonymous" and gene != "TP53":
            n_syn += 1
    sums, seen, anyone = {}, {}, {}
    for (gene, sample, annot), n in sorted(group.items()):
        if gene not in in_model:
            continue
        anyone.setdefault(gene, set()).add(sample)
        if annot in OBS_CLASSES:
            sums[(gene, annot)] = sums.get((gene, annot), 0) + min(n, max_muts_per_gene_per_sample)
        for cls, annots in N_SAMP_CLASSES.items():
            if annot in annots:
                seen.setdefault((gene, cls), set()).add(sample)
    return dict(obs={k: int(v) for k, v in sums.items()}, n_samp={k: len(v) for k, v in seen.items()}, n_syn=n_syn,
                blacklist=blacklist, pairs={g: len(v) for g, v in anyone.items()})
