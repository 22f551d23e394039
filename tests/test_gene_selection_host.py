"""CPU-only checks of the gene route's dN/dS correction and selection tests (dig_gene_selection): the plane table, the exported
symbols, the argument checks of the `_host` twin, the run_gene_model / geneDriver switches and the frame-level functions'
KeyError on a missing input column.  None of them needs a GPU."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from digdriver_amd import _lib

CLASSES = ("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")
WANT_PLANES = (["T_SYN", "MRFOLD"] + ["EXP_%s_ML" % c for c in CLASSES] + ["PVAL_%s_BURDEN_DNDS" % c for c in CLASSES]
               + ["PVAL_%s_SEL_NB" % c for c in ("SYN", "MIS", "TRUNC", "NONSYN")]
               + ["PVAL_%s_SEL_PG" % c for c in ("SYN", "MIS", "NONS", "NONSYN")]
               + ["SEL_%s" % c for c in CLASSES] + ["PVAL_%s_SEL" % c for c in CLASSES])


def test_sel_planes_are_the_34_names_in_order():
    assert len(WANT_PLANES) == 34
    assert list(_lib.SEL_PLANES) == WANT_PLANES
    from digdriver_amd import engine
    assert engine.SEL_PLANES is _lib.SEL_PLANES


def test_both_symbols_are_exported():
    lib = _lib.load()
    for sym in ("dig_gene_selection", "dig_gene_selection_host"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    assert _lib._SIGNATURES["dig_gene_selection"][-1] is ctypes.c_void_p        # stream
    assert _lib._SIGNATURES["dig_gene_selection_host"][-1] is ctypes.c_int      # device


@pytest.mark.parametrize("over, fragment", [({3: 5, 6: 2, 7: 2}, "n_pi: 4 or 6"), ({3: 6, 6: -1, 7: 2}, "G, C >= 0")])
def test_host_twin_refuses_bad_arguments_before_any_device_call(over, fragment):
    lib = _lib.load()
    buf = np.zeros(512)
    args = [_lib.host_ptr(buf) if t is ctypes.c_void_p else 0 for t in _lib._SIGNATURES["dig_gene_selection_host"]]
    for i, v in over.items():
        args[i] = v
    rc = lib.dig_gene_selection_host(*args)
    msg = _lib.last_error()
    assert rc == -1, (rc, msg)
    assert fragment in msg and "dig_gene_selection_host" in msg, msg


def test_host_twin_refuses_null_pointers():
    lib = _lib.load()
    rc = lib.dig_gene_selection_host(None, None, None, 6, None, None, 2, 2, 0)
    assert rc == -1 and "non-null pointers" in _lib.last_error()
    assert lib.dig_gene_selection_host(None, None, None, 4, None, None, 0, 3, 0) == 0         # nothing to do


def test_run_gene_model_has_selection_off_by_default():
    from digdriver_amd.driver_model import transfer_tools as tt
    par = inspect.signature(tt.run_gene_model).parameters
    assert par["selection"].default is False
    assert par["pval_burden_dnds"].default is True and par["pval_sel"].default is True


def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gene_driver_parser_accepts_the_selection_flags():
    cli = _cli()
    a = cli.parse_args("geneDriver muts.tsv model.h5 --outpfx x --outdir y --selection --no-pval-sel")
    assert a.selection is True and a.pval_sel is False and a.pval_burden_dnds is True
    a = cli.parse_args("geneDriver muts.tsv model.h5 --outpfx x --outdir y --selection --no-pval-burden-dnds")
    assert a.selection is True and a.pval_sel is True and a.pval_burden_dnds is False
    a = cli.parse_args("geneDriver muts.tsv model.h5 --outpfx x --outdir y")
    assert a.selection is False and a.pval_sel is True and a.pval_burden_dnds is True


def test_frame_functions_exist_and_raise_keyerror_without_pi_syn():
    from digdriver_amd.driver_model import transfer_tools as tt
    n = 4
    cols = {"ALPHA": np.full(n, 3.0), "THETA": np.full(n, 2.0)}
    for c in CLASSES:
        cols["Pi_" + c] = np.full(n, 0.01)
        cols["OBS_" + c] = np.arange(n, dtype=float)
        cols["EXP_" + c] = np.full(n, 0.06)
    frame = pd.DataFrame(cols, index=["G%d" % i for i in range(n)]).drop(columns=["Pi_SYN"])
    calls = [lambda d: tt.gene_expected_muts_dnds(d), lambda d: tt.gene_pvalue_burden_dnds(d), lambda d: tt.gene_pvalue_sel_nb(d),
             lambda d: tt.gene_pvalue_sel_gamma(d), lambda d: tt.selection_coefficient(d, "MIS"),
             lambda d: tt.selection_coefficient(d, "MIS", pvalue=False), lambda d: tt.gene_selection_block(d)]
    for call in calls:
        with pytest.raises(KeyError):
            call(frame.copy())
