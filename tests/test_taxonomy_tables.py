"""Taxonomy smoothing tables on the host (linnaeus_amd.loss.TaxonomySmoothingTables): what they stand for against the reference's
recorded build_distance_matrix / build_taxonomy_smoothing_matrix / generate_taxonomy_matrices (tests/golden/taxonomy_tables.npz,
written by tests/golden/gen/make_golden_taxonomy_tables.py), the refusals, the ABI of the table form, and the size at 50 000 classes."""
import ctypes as C
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import loss as LS
from tests import taxonomy_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOFT_ATOL = 2e-6  # the reference leaves a row whose fp32 sum is within 1e-6 of 1 unnormalised and divides the others by an fp32 sum;
#                   that slack plus fp32 rounding of entries <= 1 bounds the difference (rtol 0)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(REPO, "tests", "golden", "taxonomy_tables.npz"))


def forest(z, f):
    ncls = [int(c) for c in (z["big"] if f == "big" else z["forests"][f])]
    pre = "big" if f == "big" else f"f{f}"
    return ncls, [z[f"{pre}_parents_{lv}"] for lv in range(len(ncls))]


def cases(z):
    for f in range(len(z["forests"])):
        ncls, parents = forest(z, f)
        for lv in range(len(ncls)):
            yield f, lv, ncls, parents


def test_distances_equal_the_references_exactly(z):
    for f, lv, ncls, parents in cases(z):
        t = LS.build_taxonomy_smoothing_tables(parents, ncls, lv)
        assert t.depth == len(ncls) - 1 - lv and t.num_classes == ncls[lv]
        assert t.anc.dtype == torch.int32 and tuple(t.anc.shape) == (t.depth, ncls[lv])
        assert np.array_equal(R.distances(t.anc.numpy()), z[f"f{f}_l{lv}_dist"]), (f, lv)  # inf == inf included
    ncls, parents = forest(z, "big")
    t = LS.build_taxonomy_smoothing_tables(parents, ncls, 0)
    assert np.array_equal(R.distances(t.anc.numpy()), z["big_dist"])
    assert np.isinf(z["big_dist"]).any() and (z["big_dist"] == 6.0).any()  # the fixture holds disconnected pairs and the full height


def test_soft_labels_match_the_references_matrices(z):
    worst = 0.0
    fallback_rows = 0
    for f, lv, ncls, parents in cases(z):
        for s, (alpha, beta, ur) in enumerate(R.SETTINGS):
            t = LS.build_taxonomy_smoothing_tables(parents, ncls, lv, alpha, beta, ur)
            assert t.val.dtype == torch.float32 and tuple(t.val.shape) == (ncls[lv], t.depth + 2)
            got, want = R.dense(t.anc.numpy(), t.val.numpy()), z[f"f{f}_l{lv}_s{s}_soft"]
            err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
            worst = max(worst, err)
            assert err <= SOFT_ATOL, (f, lv, s, err)
            if s == 4 and t.depth:  # beta = 20: every row's weight sum is far below 1e-9 -> all uniform, disconnected classes included
                assert np.array_equal(t.val.numpy()[:, 1:], np.full((ncls[lv], t.depth + 1), np.float32(alpha / (ncls[lv] - 1))))
                fallback_rows += ncls[lv]
    ncls, parents = forest(z, "big")
    alpha, beta, ur = R.SETTINGS[0]
    t = LS.build_taxonomy_smoothing_tables(parents, ncls, 0, alpha, beta, ur)
    err = np.abs(R.dense(t.anc.numpy(), t.val.numpy()).astype(np.float64) - z["big_soft"].astype(np.float64)).max()
    worst = max(worst, err)
    print(f"taxonomy tables vs the reference's matrices: max abs difference {worst:.3e} (bound {SOFT_ATOL:g})")
    assert err <= SOFT_ATOL and fallback_rows > 0


def test_rows_sum_to_one_in_fp64_before_rounding(z):
    for f, lv, ncls, parents in cases(z):
        for alpha, beta, ur in R.SETTINGS:
            t = LS.build_taxonomy_smoothing_tables(parents, ncls, lv, alpha, beta, ur, keep_fp64=True)
            assert t.val64.dtype == np.float64
            k = R.heights(t.anc.numpy())
            counts = np.stack([(k == j).sum(1) for j in range(t.depth + 2)], 1)
            assert np.array_equal(counts, t.counts), (f, lv)  # the descendant counts are the dense matrix's multiplicities
            assert np.abs((t.val64 * t.counts).sum(1) - 1.0).max() <= 1e-12, (f, lv, alpha, beta, ur)
            assert np.array_equal(t.val64.astype(np.float32), t.val.numpy())  # rounded once


def test_tables_from_a_tree_equal_tables_from_parent_arrays(z):
    keys = [str(k) for k in z["keys"]]
    for f, lv, ncls, parents in cases(z):
        a = LS.build_taxonomy_smoothing_tables(parents, ncls, lv, 0.3, 0.25, False)
        b = LS.taxonomy_smoothing_tables_from_tree(R.Tree(parents, keys, ncls), keys[lv], 0.3, 0.25, False)
        assert torch.equal(a.anc, b.anc) and torch.equal(a.val, b.val)
    with pytest.raises(KeyError):
        LS.taxonomy_smoothing_tables_from_tree(R.Tree(parents, keys, ncls), "taxa_L99")


def stub_config(keys, flags, alpha, beta, ur, fb):
    ts = SimpleNamespace(ENABLED=list(flags), ALPHA=alpha, BETA=beta, UNIFORM_ROOTS=ur, FALLBACK_TO_UNIFORM=fb)
    return SimpleNamespace(DATA=SimpleNamespace(TASK_KEYS_H5=list(keys)), LOSS=SimpleNamespace(TAXONOMY_SMOOTHING=ts))


def test_generate_taxonomy_tables_takes_the_references_decisions(z):
    keys = [str(k) for k in z["keys"]]
    ncls, parents = forest(z, 0)
    tree, nc = R.Tree(parents, keys, ncls), dict(zip(keys, ncls))
    for g in (0, 1):
        c = z[f"gen{g}_cfg"]
        cfg = stub_config(keys, [bool(x) for x in c[4:]], float(c[0]), float(c[1]), bool(c[2]), bool(c[3]))
        got = LS.generate_taxonomy_tables(cfg, tree, nc)
        assert sorted(got) == [str(t) for t in z[f"gen{g}_tasks"]], g  # which tasks get tables, which are skipped
        for t, tab in got.items():
            assert isinstance(tab, LS.TaxonomySmoothingTables)
            err = np.abs(R.dense(tab.anc.numpy(), tab.val.numpy()).astype(np.float64) - z[f"gen{g}_{t}"]).max()
            assert err <= SOFT_ATOL, (g, t, err)
        if g == 0:  # the top level has no parent links: FALLBACK_TO_UNIFORM makes it the all-uniform matrix, as depth-0 tables
            assert got[keys[-1]].depth == 0 and got[keys[0]].depth == 3
    assert "taxa_L40" not in z["gen1_tasks"] and "taxa_L20" not in z["gen1_tasks"]  # no fallback -> skipped; flag off -> skipped
    # a task with one class, or without a class count, is skipped
    cfg = stub_config(keys, [True] * 4, 0.1, 1.0, True, True)
    assert sorted(LS.generate_taxonomy_tables(cfg, tree, {keys[0]: ncls[0], keys[1]: 1})) == [keys[0]]
    assert LS.generate_taxonomy_tables(stub_config(keys, [False] * 4, 0.1, 1.0, True, True), tree, nc) == {}


def test_refusals():
    chain = [np.zeros(4, np.int64)] + [np.zeros(1, np.int64)] * 8
    with pytest.raises(ValueError, match="at least 2 classes"):
        LS.build_taxonomy_smoothing_tables([np.array([-1])], [1], 0)
    with pytest.raises(L.LnxError, match="LNX_TAX_MAX_DEPTH"):
        LS.build_taxonomy_smoothing_tables(chain + [np.zeros(1, np.int64)], [4] + [1] * 9, 0)  # depth 9
    assert LS.build_taxonomy_smoothing_tables(chain, [4] + [1] * 8, 0).depth == 8
    with pytest.raises(ValueError, match=r"alpha must be in \[0, 1\], got 1.5"):
        LS.build_taxonomy_smoothing_tables([np.array([0, 0]), np.array([-1])], [2, 1], 0, alpha=1.5)
    with pytest.raises(ValueError, match="beta must be non-negative, got -0.5"):
        LS.build_taxonomy_smoothing_tables([np.array([0, 0]), np.array([-1])], [2, 1], 0, beta=-0.5)
    with pytest.raises(ValueError, match="parent index outside"):
        LS.build_taxonomy_smoothing_tables([np.array([0, 3]), np.array([-1, -1])], [2, 2], 0)
    with pytest.raises(ValueError, match="parent index outside"):
        LS.build_taxonomy_smoothing_tables([np.array([0, -2]), np.array([-1, -1])], [2, 2], 0)
    with pytest.raises(ValueError, match="entries"):
        LS.build_taxonomy_smoothing_tables([np.array([0, 0, 0]), np.array([-1, -1])], [2, 2], 0)


def test_criterion_in_table_form_has_the_matrix_forms_surface():
    t = LS.build_taxonomy_smoothing_tables([np.array([0, 0, 1, -1]), np.array([-1, -1])], [4, 2], 0)
    crit = LS.TaxonomyAwareLabelSmoothingCE.from_tables(t, weight=torch.ones(4), apply_class_weights=True, ignore_index=0)
    assert crit.soft_labels is None and crit.num_classes == 4 and crit.validate_targets and crit.ignore_index == 0
    assert crit.weight is crit.class_weight and crit.apply_class_weights and crit.config is None
    sd = crit.state_dict()
    assert sorted(sd) == ["class_weight", "tax_anc", "tax_val"] and sd["tax_anc"].dtype == torch.int32
    assert LS.convert_criterion(crit) is crit
    cfg = SimpleNamespace(LOSS=SimpleNamespace(GRAD_WEIGHTING=SimpleNamespace(CLASS=SimpleNamespace(TRAIN=False, VAL=False))))
    built = LS.get_loss_function("TaxonomyAwareLabelSmoothing", cfg, task_key="t", taxonomy_matrices={"t": t}, ignore_index=0)
    assert built.soft_labels is None and torch.equal(built.tax_val, t.val) and built.ignore_index == 0
    with pytest.raises(TypeError):
        LS.TaxonomyAwareLabelSmoothingCE.from_tables(torch.eye(4))


def test_new_symbols_and_struct_mirrors(tmp_path):
    import shutil
    import subprocess

    lib = L.lib()
    assert hasattr(lib, "lnx_taxonomy_rows") and "lnx_taxonomy_rows" in L.EXPORTS
    assert lib.lnx_version() >= 115
    assert (L.CE_FORM_TAXONOMY, L.TAX_MAX_DEPTH) == (3, 8)
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"lnx_softce_args": L.SoftCEArgs, "lnx_hier_loss_task": L.HierLossTask, "lnx_hier_loss_args": L.HierLossArgs,
             "lnx_taxonomy_rows_args": L.TaxonomyRowsArgs}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) +
                   '    printf("softce_tail %zu\\n", offsetof(lnx_softce_args, tax_anc));\n'
                   '    printf("hier_tail %zu\\n", offsetof(lnx_hier_loss_task, tax_anc));\n'
                   '    printf("form %d depth %d\\n", LNX_CE_FORM_TAXONOMY, LNX_TAX_MAX_DEPTH);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got = dict(line.split() for line in out[:-1])
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert int(got["softce_tail"]) == L.SoftCEArgs.tax_anc.offset and int(got["hier_tail"]) == L.HierLossTask.tax_anc.offset
    assert out[-1] == "form 3 depth 8"
    assert C.sizeof(L.SoftCEArgs) * 8 < 4096 and C.sizeof(L.HierLossArgs) < 4096  # both travel by value in the kernel-argument segment


def bad_argument_cases():
    """(entry point, call, words of the message): checked on the host before any launch, so the fake pointers are never read"""
    fake = C.c_void_p(0x1000)

    def softce(**kw):
        a = L.SoftCEArgs()
        a.B, a.C, a.logits, a.ld, a.target, a.scale, a.ignore_index = 2, 5, fake, 5, fake, 1.0, -1
        a.form, a.tax_anc, a.tax_val, a.tax_depth = L.CE_FORM_TAXONOMY, fake, fake, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def hier(**kw):
        a = L.HierLossArgs()
        a.B, a.n_tasks, a.prob, a.weights, a.ws, a.out, a.counts = 2, 1, 1.0, fake, fake, fake, fake
        k = a.task[0]
        k.logits, k.ld, k.C, k.target, k.ignore_index = fake, 5, 5, fake, -1
        k.form, k.tax_anc, k.tax_val, k.tax_depth = L.CE_FORM_TAXONOMY, fake, fake, 2
        for key, v in kw.items():
            setattr(k, key, v)
        return a

    for kw, words in (({"soft": fake}, b"excludes a [C, C] soft matrix"), ({"tax_depth": 9}, b"tax_depth=9"), ({"tax_val": None}, b"needs tax_val"),
                      ({"tax_anc": None}, b"needs tax_val"), ({"smoothing": 0.1}, b"no uniform smoothing"), ({"form": 0}, b"belong to form 3")):
        yield "lnx_softce", (lambda lib, kw=kw: lib.lnx_softce(C.byref(softce(**kw)), None)), words
        yield "lnx_softce_multi", (lambda lib, kw=kw: lib.lnx_softce_multi(C.byref(softce(**kw)), 1, None)), words
        yield "lnx_hier_loss_fwd", (lambda lib, kw=kw: lib.lnx_hier_loss_fwd(C.byref(hier(**kw)), None)), words
        yield "lnx_hier_loss_bwd", (lambda lib, kw=kw: lib.lnx_hier_loss_bwd(C.byref(hier(**kw)), fake, None)), words

    def rows(**kw):
        a = L.TaxonomyRowsArgs()
        a.C, a.depth, a.anc, a.val, a.n, a.out, a.ldo, a.what = 5, 2, fake, fake, 5, fake, 5, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, words in (({"depth": 9}, b"depth=9"), ({"val": None}, b"need val"), ({"anc": None}, b"null anc"), ({"ldo": 4}, b"ldo=4"),
                      ({"what": 2}, b"what=2"), ({"n": 0}, b"n=0")):
        yield "lnx_taxonomy_rows", (lambda lib, kw=kw: lib.lnx_taxonomy_rows(C.byref(rows(**kw)), None)), words


def test_argument_checks_refuse_before_any_launch():
    lib = L.lib()
    for who, call, words in bad_argument_cases():
        assert call(lib) != 0, (who, words)
        msg = lib.lnx_last_error()
        assert who.encode() in msg and words in msg, (who, words, msg)


def test_tables_at_50000_classes_stay_small_and_build_fast():
    rng = np.random.default_rng(5)
    ncls = [50_000, 6_000, 700, 80, 9]
    parents = [rng.integers(0, ncls[lv + 1], ncls[lv]) for lv in range(4)]
    t0 = time.perf_counter()
    t = LS.build_taxonomy_smoothing_tables(parents, ncls, 0, 0.1, 1.0, True)
    dt = time.perf_counter() - t0
    # 4 * (4 * 50 000 + 6 * 50 000) = 2 000 000 bytes, against 10 GB for the matrix
    assert t.depth == 4 and t.nbytes == 2_000_000 and t.nbytes < 2 * 2 ** 20 and t.matrix_bytes == 10_000_000_000
    assert dt < 1.0, dt
    rows = np.array([0, 17, 49_999])
    assert np.abs(R.dense(t.anc.numpy(), t.val.numpy().astype(np.float64), rows).sum(1) - 1.0).max() < 1e-5
