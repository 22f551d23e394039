"""Inputs shared by test_gpu_overlap_join.py and test_host_tools.py: one small block table and the mutation rows joined with it.
No test in here."""
import numpy as np


def block_table():
    """40 blocks (chromosome id, start, end: half-open) on the chromosome ids 1, 2 and 5, in the order a caller might give them."""
    rows = [(1, 100 + 100 * k, 200 + 100 * k) for k in range(8)]                   # back to back: [100, 200), [200, 300), ...
    rows += [(1, 120, 180), (1, 130, 140), (1, 250, 650), (1, 260, 270)]            # nested, two deep; one block over five others
    rows += [(1, 900, 900)]                                                          # zero-length: joined as [900, 901)
    rows += [(2, 5000 - 300 * k, 5200 - 300 * k + 40 * (k % 3)) for k in range(14)]  # chromosome 2 with the starts descending
    rows += [(5, 50 * k, 50 * k + 120) for k in range(13)]                           # staggered: every base under two or three blocks
    chrom, start, end = (np.array(x, np.int64) for x in zip(*rows))
    assert len(rows) == 40
    return chrom, start, end


SPANS_THREE = 6                                                                      # the row of mutation_rows over three blocks


def mutation_rows():
    """About 200 rows (chromosome id, start, end: half-open): the edges of [100, 200) on chromosome 1 from either side, one row
    over exactly three blocks of chromosome 2, rows on the chromosome ids 3 and 7 that no block has, zero-length rows."""
    rows = [(1, 99, 100), (1, 100, 101), (1, 199, 200), (1, 200, 201), (1, 899, 900), (1, 900, 901), (2, 4150, 4950), (3, 150, 160),
            (7, 5000, 5001), (5, 0, 0), (5, 731, 731), (1, 901, 950)]
    rng = np.random.RandomState(11)
    for _ in range(190):
        c = (1, 2, 5, 3)[rng.randint(4)]
        s = int(rng.randint(0, 1000) if c != 2 else rng.randint(1000, 5400))
        rows.append((c, s, s + int(rng.randint(0, 60))))
    return tuple(np.array(x, np.int64) for x in zip(*rows))
