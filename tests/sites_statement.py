"""The plain statement of engine.site_counts (dig_site_match_count / keys + a key sort + dig_site_counts) in pandas, nothing shared with
the product: per cohort the inner merge of the cohort's rows with the site table on (pos, end, attr) and the group-by per element,
as mutation_tools.tabulate_nonc_mutations_at_sites states them on the nine label columns."""
import numpy as np
import pandas as pd


def site_counts(site_pos, site_end, site_attr, site_elt, row_pos, row_end, row_attr, row_sample, row_cohort, sample_offsets, E, C,
                device=0):
    """dict(obs_snv, obs_samples), int32 [E, C], from host arrays.  A negative attr matches nothing."""
    sites = pd.DataFrame({"pos": np.asarray(site_pos), "end": np.asarray(site_end), "attr": np.asarray(site_attr),
                          "ELT": np.asarray(site_elt)})
    rows = pd.DataFrame({"pos": np.asarray(row_pos), "end": np.asarray(row_end), "attr": np.asarray(row_attr),
                         "SAMPLE": np.asarray(row_sample), "cohort": np.asarray(row_cohort)})
    obs_snv, obs_samples = np.zeros((E, C), np.int32), np.zeros((E, C), np.int32)
    for c in range(C):
        mine = rows[(rows.cohort == c) & (rows.attr >= 0)]
        at_sites = mine.merge(sites, on=["pos", "end", "attr"], how="inner")
        for elt, group in at_sites.groupby("ELT"):
            obs_snv[elt, c] = len(group)
            obs_samples[elt, c] = len(set(group.SAMPLE))
    return dict(obs_snv=obs_snv, obs_samples=obs_samples)
