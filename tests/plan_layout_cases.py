"""What lnx_plan_create decides on the host, for a list of configurations: the parameter inventory, the workspace and mask sizes, the
DropPath call count, the logits layout and the backward segment of every parameter.  All integers, all functions of the configuration
and the environment only (no device is touched), so tests/golden/plan_layout.json pins them: tests/golden/gen/make_plan_layout.py
writes what measure() returns, tests/test_plan_layout.py compares."""
import ctypes as C
import hashlib
import os

from linnaeus_amd import _lib as L
from linnaeus_amd.model import _Cfg

BASE = dict(
    dtype=L.BF16, batch=2, img_h=64, img_w=64, in_chans=3, dims=[32, 64, 128, 256], conv_depths=[1, 2], rope_depths=[2, 1],
    rope_heads=[2, 4], mlp_hidden=[512, 1024], n_meta=2, meta_dims=[4, 1], only_last_cls=0, n_tasks=2,
    task_classes=[10, 13],  # 13: a padded logits row
    inference=0, recompute=0, fp8=0, rope_mode=L.ROPE_COS,
)

# name -> (fields changed against BASE, environment switches set)
CONFIGS = {
    "base": ({}, {}),
    "fp32": ({"dtype": L.F32}, {}),
    "inference": ({"inference": 1}, {}),
    "recompute": ({"recompute": 1}, {}),
    "rotate": ({"rope_mode": L.ROPE_ROTATE}, {}),
    "only_last_cls": ({"only_last_cls": 1}, {}),
    "no_meta": ({"n_meta": 0, "meta_dims": []}, {}),
    "no_tasks": ({"n_tasks": 0, "task_classes": []}, {}),
    "img_64x96": ({"img_w": 96}, {}),
    "in_chans_4": ({"in_chans": 4}, {}),
    "no_conv_blocks": ({"conv_depths": [0, 0]}, {}),
    "inference_rotate": ({"inference": 1, "rope_mode": L.ROPE_ROTATE}, {}),
    "recompute_fp8": ({"recompute": 1, "fp8": 1}, {}),
    "fp32_recompute": ({"dtype": L.F32, "recompute": 1}, {}),
    "fp8": ({"fp8": 1}, {}),
    "fp8_dgrad_off": ({"fp8": 1}, {"LNX_FP8_DGRAD": "0"}),
    # fused conv blocks at C = 96 (resident weights) and C = 192 (streamed weights), and a RoPE stage (C = 64) the one-launch
    # metadata chain does not carry beside one (C = 128) it does
    "fused_mixed_chain": ({"dims": [96, 192, 64, 128], "rope_heads": [1, 2]}, {}),
    "unfused_conv": ({"dims": [256, 512, 256, 512], "rope_heads": [4, 4]}, {}),
    "no_fused_mlp": ({}, {"LNX_NO_FUSED_MLP": "1"}),
    "no_fused_ln": ({}, {"LNX_NO_FUSED_LN": "1"}),
}

# every switch plan creation (or a size query it calls) reads: cleared around a measurement unless the configuration sets it
SWITCHES = ("LNX_META_CHAIN", "LNX_LN_DEFER", "LNX_FREQ_DEFER", "LNX_FP8_DGRAD", "LNX_NO_FUSED_MLP", "LNX_FUSED_MLP_MAXC", "LNX_NO_FUSED_LN",
            "LNX_CM_NW")


def _cfg(fields):
    cfg = _Cfg()
    for k, v in {**BASE, **fields}.items():
        if isinstance(v, list):
            arr = getattr(cfg, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(cfg, k, v)
    return cfg


def measure(name):
    fields, env = CONFIGS[name]
    lib = L.lib()
    lib.lnx_plan_param_name.restype = C.c_char_p
    for f in ("lnx_plan_param_numel", "lnx_plan_workspace_bytes", "lnx_plan_dropout_bytes", "lnx_plan_attn_dropout_bytes", "lnx_plan_logits_numel",
              "lnx_plan_logits_offset"):
        getattr(lib, f).restype = C.c_int64
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    h = C.c_void_p()
    try:
        cfg = _cfg(fields)
        assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, lib.lnx_last_error()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    try:
        n = lib.lnx_plan_num_params(h)
        params = [f"{lib.lnx_plan_param_name(h, i).decode()}:{lib.lnx_plan_param_numel(h, i)}" for i in range(n)]
        buf = (C.c_int * n)()
        segments = []
        for seg in range(4):
            cnt = lib.lnx_plan_segment_params(h, seg, buf, n)
            assert 0 <= cnt <= n
            segments.append([buf[j] for j in range(cnt)])
        out = {
            "params_sha256": hashlib.sha256("\n".join(params).encode()).hexdigest(),
            "num_params": n,
            "workspace_bytes": lib.lnx_plan_workspace_bytes(h),
            "dropout_bytes": lib.lnx_plan_dropout_bytes(h),
            "attn_dropout_bytes": lib.lnx_plan_attn_dropout_bytes(h),
            "num_drop_calls": lib.lnx_plan_num_drop_calls(h),
            "logits_numel": lib.lnx_plan_logits_numel(h),
            "logits": [[lib.lnx_plan_logits_offset(h, t), lib.lnx_plan_logits_ld(h, t)] for t in range(cfg.n_tasks)],
            "segments": segments,
        }
        if name == "base":
            out["params"] = params
        return out
    finally:
        lib.lnx_plan_destroy(h)
