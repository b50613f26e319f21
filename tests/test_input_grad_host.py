"""Input gradients on the host (no GPU): what lnx_stem_dgrad / lnx_col2im_stem / lnx_meta_input_grad refuse before any launch, and
what lnx_plan_set_input_grads does to a plan's cut and workspace (lnx_plan_create and the setters need no device).  The refusal of
lnx_plan_set_input_grads AFTER lnx_plan_bind needs a bound plan, so a device: tests/test_gpu_input_grad_model.py checks it."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from tests.cases import CASES, make_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = {"tiny_a": 64, "tiny_b": 96, "tiny_c": 64, "sm": 224}
FAKE = 0x10000  # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _model(name):
    spec = CASES[name]
    return build_model(make_config(spec, IMG[name]), num_classes={t: c for t, c in spec.heads})


def _err():
    return L.lib().lnx_last_error().decode()


def test_version_and_exports():
    lib = L.lib()
    assert lib.lnx_version() >= 121
    for name in ("lnx_stem_dgrad_ok", "lnx_stem_dgrad", "lnx_col2im_stem", "lnx_meta_input_grad", "lnx_plan_set_input_grads", "lnx_plan_input_grads",
                 "lnx_plan_bind_input_grads"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"lnx_stem_dgrad_args": L.StemDgradArgs, "lnx_meta_input_grad_args": L.MetaInputGradArgs}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))


def test_stem_dgrad_ok_mirrors_the_forward():
    lib = L.lib()
    for cout in (32, 64, 96, 128, 160, 192, 256, 384):
        for cin in (0, 1, 3, 4, 5):
            for hw in ((224, 224), (12, 20), (6, 8), (8, 6)):
                want = cin in (1, 3, 4) and hw[0] % 4 == 0 and hw[1] % 4 == 0 and cout in (96, 128, 192, 256)
                assert bool(lib.lnx_stem_fwd_ok(L.BF16, cin, hw[0], hw[1], cout)) == want  # (the forward's own rule, restated above)
                for dt in (L.BF16, L.F32):
                    assert bool(lib.lnx_stem_dgrad_ok(dt, cin, hw[0], hw[1], cout)) == want, (dt, cin, hw, cout)
                assert not lib.lnx_stem_dgrad_ok(7, cin, hw[0], hw[1], cout)


def _dgrad_args(**kw):
    a = L.StemDgradArgs()
    a.dtype, a.B, a.Cin, a.H, a.W, a.Cout = L.BF16, 2, 3, 8, 8, 96
    a.dy, a.ldy, a.w, a.dx = FAKE, 96, FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(dy=None), "null operand"), (dict(w=None), "null operand"), (dict(dx=None), "null operand"),
    (dict(H=6), "multiples of 4"), (dict(W=10), "multiples of 4"), (dict(dtype=7), "unsupported dtype"),
    (dict(Cout=64, ldy=64), "unsupported geometry"), (dict(Cin=5), "unsupported geometry"), (dict(ldy=100), "ldy"), (dict(ldy=64), "ldy"),
    (dict(dx=FAKE + 4), "16-byte aligned"),
])
def test_stem_dgrad_refusals(kw, word):
    lib = L.lib()
    a = _dgrad_args(**kw)
    assert lib.lnx_stem_dgrad(C.byref(a), None) != 0
    assert "lnx_stem_dgrad" in _err() and word in _err(), _err()


def test_stem_dgrad_null_args():
    assert L.lib().lnx_stem_dgrad(None, None) != 0
    assert "lnx_stem_dgrad: null operand" in _err()


@pytest.mark.parametrize("args,word", [
    ((None, L.BF16, 64, 1, 3, 8, 8, FAKE), "null operand"), ((FAKE, L.BF16, 64, 1, 3, 8, 8, None), "null operand"),
    ((FAKE, 7, 64, 1, 3, 8, 8, FAKE), "unsupported dtype"), ((FAKE, L.F32, 64, 1, 3, 6, 8, FAKE), "multiples of 4"),
    ((FAKE, L.F32, 64, 1, 3, 8, 10, FAKE), "multiples of 4"), ((FAKE, L.F32, 32, 1, 3, 8, 8, FAKE), "ldp"),
    ((FAKE, L.F32, 64, 1, 3, 8, 8, FAKE + 8), "16-byte aligned"),
])
def test_col2im_stem_refusals(args, word):
    assert L.lib().lnx_col2im_stem(*args, None) != 0
    assert "lnx_col2im_stem" in _err() and word in _err(), _err()


def _mig_heads(specs):
    arr = (L.MetaInputGradArgs * len(specs))()
    for a, (B, Cc, dim, off) in zip(arr, specs):
        a.B, a.C, a.dim, a.off, a.dp0, a.lddp0, a.w0, a.ldw0 = B, Cc, dim, off, FAKE, Cc, FAKE, 16
    return arr


def test_meta_input_grad_refusals():
    lib = L.lib()
    one = _mig_heads([(4, 128, 3, 0)])
    assert lib.lnx_meta_input_grad(None, 1, FAKE, 5, 0, None) != 0 and "no heads" in _err()
    assert lib.lnx_meta_input_grad(one, 0, FAKE, 5, 0, None) != 0 and "no heads" in _err()
    assert lib.lnx_meta_input_grad(one, 1, None, 5, 0, None) != 0 and "dmeta is NULL" in _err()
    nine = _mig_heads([(4, 128, 1, i) for i in range(9)])
    assert lib.lnx_meta_input_grad(nine, 9, FAKE, 9, 0, None) != 0 and "LNX_MAX_META" in _err()
    for spec, word in (((4, 128, 17, 0), "dim"), ((4, 128, 0, 0), "dim"), ((4, 128, 3, 3), "metadata slice"), ((0, 128, 3, 0), "B=0")):
        assert lib.lnx_meta_input_grad(_mig_heads([spec]), 1, FAKE, 5, 0, None) != 0 and word in _err(), (spec, _err())
    null_dp = _mig_heads([(4, 128, 3, 0)])
    null_dp[0].dp0 = None
    assert lib.lnx_meta_input_grad(null_dp, 1, FAKE, 5, 0, None) != 0 and "null operand" in _err()
    overlap = _mig_heads([(4, 128, 3, 0), (4, 128, 2, 2)])
    assert lib.lnx_meta_input_grad(overlap, 2, FAKE, 5, 0, None) != 0 and "overlap" in _err()


def _plan(model, batch, img, train=True, recompute=False):
    lib = L.lib()
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    cfg = model._make_cfg(batch, img, img, train, recompute)
    h = C.c_void_p()
    L.check(lib.lnx_plan_create(C.byref(cfg), C.byref(h)), "lnx_plan_create")
    return h


def _unit(h):
    lib = L.lib()
    return lib.lnx_plan_unit_name(h, lib.lnx_plan_first_trained_unit(h)).decode()


def test_plan_refusals():
    lib = L.lib()
    h = _plan(_model("tiny_c"), 2, 64)  # no metadata components
    try:
        assert lib.lnx_plan_set_input_grads(h, 0, 1) != 0
        assert "lnx_plan_set_input_grads" in _err() and "without metadata components" in _err()
        assert lib.lnx_plan_input_grads(h) == 0
        assert lib.lnx_plan_set_input_grads(h, 1, 0) == 0 and lib.lnx_plan_input_grads(h) == 1
        assert lib.lnx_plan_bind_input_grads(h, None, FAKE) != 0 and "want_meta" in _err()
        assert lib.lnx_plan_bind_input_grads(h, FAKE + 4, None) != 0 and "aligned" in _err()
        assert lib.lnx_plan_bind_input_grads(h, FAKE, None) == 0  # callable before any backward (and before the bind)
        assert lib.lnx_plan_bind_input_grads(h, None, None) == 0
    finally:
        lib.lnx_plan_destroy(h)
    h = _plan(_model("tiny_a"), 2, 64, train=False)  # training-only calls on an inference plan
    try:
        assert lib.lnx_plan_set_input_grads(h, 1, 0) != 0 and "lnx_plan_set_input_grads" in _err() and "inference plan" in _err()
        assert lib.lnx_plan_bind_input_grads(h, FAKE, None) != 0 and "lnx_plan_bind_input_grads" in _err() and "inference plan" in _err()
    finally:
        lib.lnx_plan_destroy(h)
    assert lib.lnx_plan_set_input_grads(None, 1, 0) != 0 and "null plan" in _err()
    assert lib.lnx_plan_input_grads(None) < 0


def test_all_frozen_mask_needs_a_flag_and_moves_the_cut_to_the_source():
    lib = L.lib()
    model = _model("tiny_a")
    n = len(model.plan_units()["names"])
    h = _plan(model, 2, 64)
    try:
        assert lib.lnx_plan_set_trainable(h, bytes(n)) != 0 and "all zero" in _err()  # as before: nothing trains, nothing is differentiated
        assert lib.lnx_plan_set_input_grads(h, 1, 0) == 0
        assert lib.lnx_plan_set_trainable(h, bytes(n)) == 0, _err()
        assert _unit(h) == "stem" and lib.lnx_plan_first_trained_unit(h) == 0
        assert lib.lnx_plan_set_input_grads(h, 0, 1) == 0  # only the metadata: the token units and everything behind them
        assert _unit(h) == "tokens_1" and lib.lnx_plan_input_grads(h) == 2
        assert lib.lnx_plan_set_input_grads(h, 0, 0) != 0 and "all zero" in _err()  # the mask in force says that nothing trains
        assert lib.lnx_plan_set_input_grads(h, 1, 1) == 0 and _unit(h) == "stem" and lib.lnx_plan_input_grads(h) == 3
    finally:
        lib.lnx_plan_destroy(h)


@pytest.mark.parametrize("name,batch", [("tiny_b", 2), ("sm", 4)])
def test_cut_and_workspace(name, batch):
    """Flags in either order with the mask; without flags the workspace is the parent's for every cut."""
    lib = L.lib()
    model = _model(name)
    img = IMG[name]
    info = model.plan_units()
    units, unit_of = info["units"], info["unit_of"]
    h = _plan(model, batch, img)
    full = int(lib.lnx_plan_workspace_bytes(h))
    lib.lnx_plan_destroy(h)
    fused = bool(lib.lnx_stem_dgrad_ok(model._dtype_code, model._in_chans, img, img, model._dims[0]))
    assert fused == (name == "sm")
    for cut_name in ("stem", "stages.1.0", "tokens_1", "stages.2.1", "mid", "tokens_2", "heads"):
        u = units.index(cut_name)
        mask = bytes(int(pu >= u) for pu in unit_of)
        h = _plan(model, batch, img)
        try:
            assert lib.lnx_plan_set_trainable(h, mask) == 0
            plain = int(lib.lnx_plan_workspace_bytes(h))
            assert _unit(h) == cut_name
            assert lib.lnx_plan_set_input_grads(h, 0, 0) == 0  # no flags: the plan as it was
            assert int(lib.lnx_plan_workspace_bytes(h)) == plain and _unit(h) == cut_name
            assert lib.lnx_plan_set_input_grads(h, 0, 1) == 0
            assert _unit(h) == units[min(u, units.index("tokens_1"))]
            if u <= units.index("tokens_1"):
                assert int(lib.lnx_plan_workspace_bytes(h)) == plain  # the metadata gradient needs no workspace of its own
            assert lib.lnx_plan_set_input_grads(h, 1, 0) == 0
            assert _unit(h) == "stem"
            with_x = int(lib.lnx_plan_workspace_bytes(h))
            # the image gradient: nothing beyond the full plan where one kernel carries the stem's geometry, else the transposed
            # weight copy and the [M0, Cin * 16] product of the two-launch fallback
            assert with_x == full if fused else with_x > full
            assert lib.lnx_plan_set_input_grads(h, 0, 0) == 0
            assert int(lib.lnx_plan_workspace_bytes(h)) == plain and _unit(h) == cut_name
        finally:
            lib.lnx_plan_destroy(h)
        # the other order: flags first, then the mask
        h = _plan(model, batch, img)
        try:
            assert lib.lnx_plan_set_input_grads(h, 1, 1) == 0
            assert lib.lnx_plan_set_trainable(h, mask) == 0
            assert _unit(h) == "stem" and int(lib.lnx_plan_workspace_bytes(h)) == with_x
        finally:
            lib.lnx_plan_destroy(h)
