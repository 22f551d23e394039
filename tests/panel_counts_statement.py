"""What the target route counts inside a sequencing panel, stated in plain Python: sets and dicts over (gene, sample, annot)
tuples.  No pandas, no numpy, no code of the route.  No test in here.

The tuples are the rows of read_mutation_file(drop_duplicates=True) in any order.  For one cohort:
  n_cds      rows of samples that are not blacklisted whose annotation is not Noncoding
  per panel  of the rows of samples that are not blacklisted whose annotation is none of Noncoding, Synonymous, Essential_Splice
             and whose gene is in the panel:
               n_mut     their number
               n_pairs   their distinct (gene, sample) pairs
               n_sample  their distinct samples
(CohortRun.panel_scale, transfer_tools.py:905-935; DigPretrain.py countMutations, :103-177.)"""

NOT_COUNTED = ("Noncoding", "Synonymous", "Essential_Splice")


def cohort_panel_counts(tuples, panels, blacklist=()):
    """tuples: (gene, sample, annot); panels: dict name -> gene list; blacklist: sample names.  Returns dict(n_cds, n_samples: the
    distinct samples of all rows, panels: dict name -> dict(n_mut, n_pairs, n_sample))."""
    black = set(blacklist)
    rows = [(g, s, a) for g, s, a in tuples if s not in black]
    out = {}
    for name, genes in panels.items():
        genes = set(genes)
        inside = [(g, s) for g, s, a in rows if a not in NOT_COUNTED and g in genes]
        out[name] = dict(n_mut=len(inside), n_pairs=len(set(inside)), n_sample=len(set(s for _, s in inside)))
    return dict(n_cds=sum(1 for _, _, a in rows if a != "Noncoding"), n_samples=len(set(s for _, s, _ in tuples)), panels=out)
