"""The other arm of the native switches (csrc/switches.h) that no GPU test set before: each arm re-runs comparisons the suite
already makes with a reference -- at their smallest shapes and at their own bars -- and proves that the arm was in force.

What an arm runs:
  EDVR tape       test_gpu_edvr._kink_free_gradient_check({}, 0, 1, 32, 48, 21, 22): all 144 parameter gradients under 1e-4 and
                  the input gradient under 5e-4 against the fp64 oracle forced onto the GPU's own activations
  estimator tape  test_gpu_estimator: test_mfdn_x4_vs_oracle_shapes at (2,5,16,48), (1,7,36,20), (1,5,12,12), test_mfdn_x2_golden,
                  test_sfdn_golden (outputs 1e-5, every parameter gradient 2e-4)
  op level        test_gpu_ops: test_tsa_gate_and_blend, test_upsample_bilinear, test_conv2d_backward, test_conv3x3_wgrad_split3

BUILD switches are part of the plan-cache key: their arms run in this process under monkeypatch.setenv.  PROCESS switches are
read once per process: each of their arms is a child, `python -m pytest <node ids> -q -x -s` with the arm in its environment,
one child after another.  A child's first test is test_arm_in_force, which exists in a child only (SWITCH_ARM_CHILD is set):
dvsr_switch_value must give the arm's value for every switch the arm sets, in the very process that then runs the arm.
Where the arm changes the tape, the plan must show it (backward launch counts above the default plan's, a refused plan, the
weight gradients' kernel and pipe); where it runs other arithmetic, the result must not be bit-equal to the default arm's,
which this process computes once (the `default_arm` fixture) and hands to the children as a file.

A child that ends on a signal, with status 134 or 139, with a HIP fault in its output or at its time limit is recorded: every
later arm test of this module then fails at once and starts nothing more on the GPU.

The first two rows of the arm table change which gradient buffer is zeroed and who accumulates, and a fresh workspace is all
zeros by luck: every EDVR tape here runs over a workspace that held NaN bit patterns (_edvr_tape).  With that, a library whose
BackBuilder::contribute skips its B_MEMSET under DVSR_FUSE_RES_BWD=0 fails that arm (input gradient NaN) and passes the default
arm; over a fresh workspace it passed both.

Wall time of this module on an MI355X machine: 67 - 69 s for the fifteen tests, 5 - 7 s per child (child start-up and the
CPU oracle, not GPU time).
"""
import collections
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_ENV = "SWITCH_ARM_CHILD"     # JSON, set by _run_child alone: which arm the child runs and what the parent computed for it
CHILD = json.loads(os.environ[CHILD_ENV]) if os.environ.get(CHILD_ENV) else None
gpu = pytest.mark.gpu

EDVR_TAPE_SHAPE = (1, 32, 48)      # the smaller shape of test_edvr_backward_kink_free_all_144_gradients
WGRAD_DESC = (2, 64, 12, 40, 64)   # N, Cin, H, W, Cout of a 3x3 stride-1 layer with W % 4 == 0: float4 staging by default

# arm -> (environment of the arm, what dvsr_switch_value must then say, the child's time limit in seconds, what the child runs
# after test_arm_in_force, how many tests that makes).  The first six letters of a node id name its module.
_EDVR = "arms::test_arm_edvr_tape"
_EST12 = "estimator::test_mfdn_x4_vs_oracle_shapes[1-5-12-12]"
_EST = ["estimator::test_mfdn_x4_vs_oracle_shapes[2-5-16-48]", "estimator::test_mfdn_x4_vs_oracle_shapes[1-7-36-20]", _EST12,
        "estimator::test_mfdn_x2_golden", "estimator::test_sfdn_golden"]
ARMS = {
    "fuse_res": ({"DVSR_FUSE_RES_BWD": "0"}, {"DVSR_FUSE_RES_BWD": 0}, 300, [_EDVR], 1),
    "unfused": ({"DVSR_FUSE_RES_BWD": "0", "DVSR_FUSE_ACT_BWD": "0"}, {"DVSR_FUSE_RES_BWD": 0, "DVSR_FUSE_ACT_BWD": 0}, 300, [_EDVR], 1),
    "fork_probe": ({"DVSR_BWD_FORK_EVERY": "1", "DVSR_BWD_PROBE": "0"}, {"DVSR_BWD_FORK_EVERY": 1, "DVSR_BWD_PROBE": 0}, 300,
                   [_EDVR, _EST12], 2),
    "tsa_up2": ({"DVSR_TSA_DUAL": "0", "DVSR_TSA_V": "1", "DVSR_UP2": "4"}, {"DVSR_TSA_DUAL": 0, "DVSR_TSA_V": 1, "DVSR_UP2": 1}, 300,
                [_EDVR, "ops::test_tsa_gate_and_blend", "ops::test_upsample_bilinear"], 1 + 4 + 12),
    "tsa_v4": ({"DVSR_TSA_V": "4"}, {"DVSR_TSA_V": 4}, 120, ["ops::test_tsa_gate_and_blend"], 4),
    "wgrad_fp32": ({"DVSR_WGRAD_SPLIT3": "0"}, {"DVSR_WGRAD_SPLIT3": 0}, 300, [_EDVR] + _EST, 1 + 5),
    "wgrad_scalar": ({"DVSR_WGRAD_WIDE": "0"}, {"DVSR_WGRAD_WIDE": 0}, 300,
                     ["ops::test_conv2d_backward", "ops::test_conv3x3_wgrad_split3", _EDVR], 13 + 6 + 1),
    "est_pads": ({"DVSR_EST_FUSE_PAD": "0"}, {"DVSR_EST_FUSE_PAD": 0}, 300, _EST, 5),
    "th8": ({"DVSR_SPLIT_TH8_FROM": "1"}, {"DVSR_SPLIT_TH8_FROM": 1}, 240,
            ["edvr::test_edvr_backward_all_grads_vs_oracle[2]", "edvr::test_edvr_split_bf16_mfma_path"], 2),
}
_MODULES = {"arms": os.path.abspath(__file__), "estimator": os.path.join(HERE, "test_gpu_estimator.py"),
            "ops": os.path.join(HERE, "test_gpu_ops.py"), "edvr": os.path.join(HERE, "test_gpu_edvr.py")}
_FAULT = []   # why nothing more may start on the GPU from this module


def _node(short):
    mod, rest = short.split("::", 1)
    return _MODULES[mod] + "::" + rest


def _wgrad_geometry(mode):
    """dvsr_conv2d_wgrad_geometry of WGRAD_DESC (no device: of the pointers only the alignment is read)."""
    from dynavsr_amd import _lib as L
    n, cin, h, w, cout = WGRAD_DESC
    d = L.Conv2dDesc(0x10000000, None, None, None, None, 0x20000000, n, cin, 0, h, w, cout, 3, 1, 1, 0, 0, 1, 0, 0, None, 0)
    geo = (ctypes.c_int * 8)()
    L.check(L.lib().dvsr_conv2d_wgrad_geometry(d, mode, 1, ctypes.byref(geo)), "dvsr_conv2d_wgrad_geometry")
    return list(geo)


def _edvr_tape(monkeypatch):
    """The kink-free gradient check of test_gpu_edvr at EDVR_TAPE_SHAPE under the switches now in force, and what it computed:
    the output, every parameter gradient, the plan's backward launch count and its work figures."""
    import torch
    import test_gpu_edvr as E
    from dynavsr_amd import engine
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    # The tape's workspace is a fresh torch.empty, which is all zeros when the allocator has just taken it from the driver: a
    # first contribution that accumulated into its gradient buffer without the memset would pass by luck.  A block of the
    # workspace's size is filled with NaN bit patterns and freed; the allocator hands that block to the check.
    nbytes = engine.get_plan(EDVR()._cfg(), *EDVR_TAPE_SHAPE).workspace_bytes(True)
    dirty = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    dirty_ptr = dirty.data_ptr()
    torch.cuda.synchronize()
    del dirty
    seen = {}
    make_net = E.make_net

    def recording_make_net(*a, **k):
        net = seen["net"] = make_net(*a, **k)
        net.register_forward_hook(lambda _m, _i, out: seen.__setitem__("y", out.detach().cpu().clone()))
        return net
    monkeypatch.setattr(E, "make_net", recording_make_net)
    E._kink_free_gradient_check({}, 0, *EDVR_TAPE_SHAPE, 21, 22)
    net = seen["net"]
    plan, ws = net._debug_ws[-1]
    assert ws.data_ptr() == dirty_ptr and ws.numel() == nbytes, "the check did not run over the dirtied workspace"
    grads = collections.OrderedDict((n, p.grad.detach().cpu().clone()) for n, p in zip(net._names, net.ordered_parameters()))
    return {"y": seen["y"], "grads": grads, "n_bwd": plan.n_backward_launches, "work": plan.work(), "cfg": net._cfg()}


def _plan_count(cfg):
    """Backward launches (p->bops.size()) of a fresh plan at EDVR_TAPE_SHAPE under the switches now in force; launches nothing."""
    from dynavsr_amd import engine
    return engine.Plan(tuple(cfg), *EDVR_TAPE_SHAPE).n_backward_launches


def _differs(a, b, what):
    """what = "y": the network outputs are not bit-equal; "wgrad": some convolution's weight gradient is not."""
    import torch
    if what == "y":
        return not torch.equal(a["y"], b["y"])
    return any(not torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"] if k.endswith(".weight"))


@pytest.fixture(scope="module")
def default_arm(tmp_path_factory):
    """The default arm, once: every switch of ARMS and of the in-process arms at its default (or the comparisons below would
    mean nothing), the EDVR tape's result in a file for the children, the default plan's backward launch count, the count
    under DVSR_FUSE_ACT_BWD=0 alone (a BUILD switch: this process can build that plan) and the float4 staging of WGRAD_DESC."""
    import torch
    from dynavsr_amd import _lib as L
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dflt = {name: d for name, _scope, d, _doc in L.switches()}
    names = sorted({k for _e, v, _t, _r, _n in ARMS.values() for k in v} | {"DVSR_FUSE_ACT_BWD", "DVSR_CONV_V1", "DVSR_BWD_STREAMS"})
    off = [k for k in names if L.switch_value(k) != dflt[k]]
    assert not off, "this module compares arms with the default arm: unset %s" % off
    with pytest.MonkeyPatch.context() as mp:
        res = _edvr_tape(mp)
        mp.setenv("DVSR_FUSE_ACT_BWD", "0")
        n_act = _plan_count(res["cfg"])
    path = str(tmp_path_factory.mktemp("switch_arms") / "default_arm.pt")
    torch.save({"y": res["y"], "grads": res["grads"]}, path)
    assert res["work"]["bwd_bf16_pipe"] > 0, "the default plan's 3x3 weight gradients run on the bf16 pipe"
    geo = {mode: _wgrad_geometry(mode) for mode in (0, 2)}
    assert geo[0][2] == 4 and geo[2][2] == 4 and geo[2][0] >= 3, geo   # float4 staging in both kernels; the split kernel
    res.update(path=path, n_act=n_act)
    return res


def _run_child(arm, default_arm, expect=None, only_in_force=False):
    """One arm in a child; returns the child's output.  `expect`: what test_arm_in_force is told to expect instead of the arm's
    own values (the device-free check that the proof can fail)."""
    if _FAULT:
        pytest.fail("nothing more starts on the GPU from this module: " + _FAULT[0])
    env, values, limit, runs, count = ARMS[arm]
    tell = {"arm": arm, "expect": values if expect is None else expect}
    if default_arm is not None:
        tell.update(default=default_arm["path"], n_default=default_arm["n_bwd"], n_act=default_arm["n_act"])
    ids = [_node("arms::test_arm_in_force")] + ([] if only_in_force else [_node(r) for r in runs])
    cmd = [sys.executable, "-m", "pytest"] + ids + ["-q", "-x", "-s"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **env, **{CHILD_ENV: json.dumps(tell)}), capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired as e:
        _FAULT.append("the child of arm %r had not ended after %d s" % (arm, limit))
        pytest.fail(_FAULT[0] + "\n" + str(e.stdout or "")[-2000:])
    out = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (134, 139) or re.search(r"illegal memory access|HSA_STATUS_ERROR|Memory access fault", out):
        _FAULT.append("the child of arm %r ended with status %d (a signal, an abort or a GPU fault)" % (arm, r.returncode))
        pytest.fail(_FAULT[0] + "\n" + out[-3000:])
    for line in out.splitlines():
        if line.lstrip(".").startswith(("kink-free gradient check", "arm ", "median rel-L2")):   # (-q -s: progress dots precede them)
            print("[%s] %s" % (arm, line.lstrip(".")))
    if expect is not None:
        return r
    assert r.returncode == 0, out[-4000:]
    m = re.search(r"\b(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 1 + (0 if only_in_force else count) and " skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
    return r


# ---- the child's half: these two tests exist in a child only ---------------------------------------------------------------
if CHILD is not None:
    def test_arm_in_force():
        """dvsr_switch_value, in the process that runs the arm, for every switch the arm sets; and what the weight-gradient
        rule answers under the two DVSR_WGRAD_* arms (no device needed)."""
        from dynavsr_amd import _lib as L
        got = {k: L.switch_value(k) for k in CHILD["expect"]}
        assert got == CHILD["expect"], (got, CHILD["expect"])
        if CHILD["arm"] == "wgrad_fp32":    # the switch changes what the plans ASK for, not the rule: mode 2 is still a split kernel
            assert _wgrad_geometry(2)[0] >= 3 and _wgrad_geometry(0)[0] == 1
        if CHILD["arm"] == "wgrad_scalar":  # float4 by default (the parent asserts it): scalar staging in the fp32 and the split kernel
            assert _wgrad_geometry(0)[2] == 0 and _wgrad_geometry(2)[2] == 0 and _wgrad_geometry(2)[0] == 3, (_wgrad_geometry(0), _wgrad_geometry(2))

    @gpu
    def test_arm_edvr_tape(monkeypatch):
        """The EDVR tape under the child's arm, and the arm's mark on the plan or on the result."""
        import torch
        arm = CHILD["arm"]
        res = _edvr_tape(monkeypatch)
        base = torch.load(CHILD["default"])
        print("arm %s: backward launches %d (default plan %d, DVSR_FUSE_ACT_BWD=0 alone %d), bwd_bf16_pipe %.3g, output bit-equal to the "
              "default arm's: %s" % (arm, res["n_bwd"], CHILD["n_default"], CHILD["n_act"], res["work"]["bwd_bf16_pipe"],
                                     not _differs(res, base, "y")))
        if arm == "fuse_res":
            assert res["n_bwd"] > CHILD["n_default"]
        if arm == "unfused":
            monkeypatch.setenv("DVSR_FUSE_ACT_BWD", "1")      # (a BUILD switch: the plan with the copies alone unfused)
            n_res = _plan_count(res["cfg"])
            print("arm unfused: DVSR_FUSE_RES_BWD=0 alone %d" % n_res)
            assert n_res > CHILD["n_default"] and res["n_bwd"] > n_res and res["n_bwd"] > CHILD["n_act"] > CHILD["n_default"]
        if arm == "tsa_up2":
            assert _differs(res, base, "y")                   # two 1x1 launches sum in another order than the dual kernel
        if arm == "wgrad_fp32":
            assert res["work"]["bwd_bf16_pipe"] == 0          # an fp32 plan: nothing of its backward on the bf16 pipe
            assert _differs(res, base, "wgrad")
        if arm == "wgrad_scalar":
            assert res["n_bwd"] == CHILD["n_default"]         # the same tape, other staging


# ---- device-free -----------------------------------------------------------------------------------------------------------
def test_every_switch_has_a_gpu_test():
    """Every row of the library's switch table is named by a GPU test module (tests/test_gpu_*.py), so that a switch added later
    without a test of its other arm fails here.  The exceptions are the DEBUG rows: they act in the trace build only and give
    wrong results on purpose."""
    import glob
    from dynavsr_amd import _lib as L
    text = ""
    for path in sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py"))):
        with open(path) as f:
            src = f.read()
        if "pytest.mark.gpu" in src:
            text += src
    rows = L.switches()
    debug = sorted(name for name, scope, _d, _doc in rows if scope == L.SW_DEBUG)
    assert debug == ["DVSR_CONV_ABLATE", "DVSR_CONV_LDS", "DVSR_WGRAD_NOFLUSH"], debug
    missing = [name for name, scope, _d, _doc in rows if scope != L.SW_DEBUG and not re.search(r"\b%s\b" % re.escape(name), text)]
    assert not missing, missing


def test_the_arm_table_names_real_switches_and_non_default_values():
    """ARMS against the library's own table and parser: every name exists, every value is what the parser makes of the arm's
    text, and none is the switch's default (an arm equal to the default arm would test nothing)."""
    from dynavsr_amd import _lib as L
    rows = {name: (i, scope, dflt) for i, (name, scope, dflt, _doc) in enumerate(L.switches())}
    for arm, (env, values, limit, runs, count) in ARMS.items():
        assert set(env) == set(values) and 0 < limit <= 300 and count >= len(runs), arm
        for name, text in env.items():
            i, scope, dflt = rows[name]
            v = ctypes.c_int()
            L.check(L.lib().dvsr_switch_parse(i, text.encode(), ctypes.byref(v)), "dvsr_switch_parse")
            assert v.value == values[name] != dflt, (arm, name, v.value, dflt)
        assert any(rows[name][1] == L.SW_PROCESS for name in env), arm   # (an arm of BUILD switches alone needs no child)


def test_a_child_with_the_wrong_expectation_fails():
    """The proof of effect can fail: a child told to expect DVSR_FUSE_RES_BWD = 1 under DVSR_FUSE_RES_BWD=0 does not pass, and
    one told the truth does.  No device: test_arm_in_force needs none."""
    r = _run_child("fuse_res", None, expect={"DVSR_FUSE_RES_BWD": 1}, only_in_force=True)
    assert r.returncode == 1 and "1 failed" in r.stdout, r.stdout[-1000:]
    _run_child("fuse_res", None, only_in_force=True)


# ---- BUILD switches: in this process -----------------------------------------------------------------------------------------
def _in_process(monkeypatch, **env):
    from dynavsr_amd import _lib as L
    if _FAULT:
        pytest.fail("nothing more starts on the GPU from this module: " + _FAULT[0])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return L


@gpu
def test_fuse_act_bwd_0_edvr_tape(default_arm, monkeypatch):
    """DVSR_FUSE_ACT_BWD=0: every activation backward a separate B_ACT launch (build_backward: act_fused, mask_op, the
    sole_producer_with_act path).  EDVR tape; the plan holds more backward launches than the default plan.
    Measured: worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; 229 backward launches, the default plan 203."""
    L = _in_process(monkeypatch, DVSR_FUSE_ACT_BWD="0")
    assert L.switch_value("DVSR_FUSE_ACT_BWD") == 0
    res = _edvr_tape(monkeypatch)
    print("arm fuse_act: backward launches %d (default plan %d)" % (res["n_bwd"], default_arm["n_bwd"]))
    assert res["n_bwd"] == default_arm["n_act"] > default_arm["n_bwd"]


@gpu
def test_conv_v1_1_edvr_tape(default_arm, monkeypatch):
    """DVSR_CONV_V1=1: the un-pipelined conv kernel for the whole plan (every `!p.use_v1 &&` branch of engine.hip: no packs, no
    mask input, no pending residual).  EDVR tape; such a plan refuses per-sample weight sets with DVSR_ERR_UNSUPPORTED, which
    the default arm accepts; the output is not bit-equal to the default arm's.
    Measured: worst parameter gradient 1.5e-6 of 1e-4, input gradient 6.2e-6 of 5e-4; 244 backward launches, the default plan 203."""
    from dynavsr_amd import engine
    L = _in_process(monkeypatch)
    cfg = default_arm["cfg"]
    assert engine.Plan(cfg, 2, 32, 48, 2, 2).weight_sets == 2
    monkeypatch.setenv("DVSR_CONV_V1", "1")
    assert L.switch_value("DVSR_CONV_V1") == 1
    h = ctypes.c_void_p()
    assert L.lib().dvsr_edvr_plan_create_ex(L.EdvrConfig(*cfg), 2, 32, 48, 2, 2, ctypes.byref(h)) == -2 and not h   # DVSR_ERR_UNSUPPORTED
    res = _edvr_tape(monkeypatch)
    print("arm conv_v1: backward launches %d (default plan %d)" % (res["n_bwd"], default_arm["n_bwd"]))
    assert _differs(res, default_arm, "y")


@gpu
def test_bwd_streams_0_edvr_and_estimator_tapes(default_arm, monkeypatch):
    """DVSR_BWD_STREAMS=0: weight gradients on the launch stream, no side stream (the ordering between the data-gradient chain,
    the weight gradients and the batched reduce).  EDVR tape and the estimator tape at (1,5,12,12); dvsr_switch_value is the
    proof: the arm moves launches between streams and changes no arithmetic.
    Measured: EDVR worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; estimator output 8.2e-7 of 1e-5, worst parameter gradient 2.2e-6 of 2e-4."""
    import test_gpu_estimator as M
    L = _in_process(monkeypatch, DVSR_BWD_STREAMS="0")
    assert L.switch_value("DVSR_BWD_STREAMS") == 0
    _edvr_tape(monkeypatch)
    M.test_mfdn_x4_vs_oracle_shapes(1, 5, 12, 12)


# ---- PROCESS switches: a child per arm -----------------------------------------------------------------------------------------
@gpu
def test_fuse_res_bwd_0_edvr_tape(default_arm):
    """DVSR_FUSE_RES_BWD=0: skip-connection gradient copies as B_COPYADD launches (BackBuilder::copyadd, contribute,
    take_pending_as_residual: which buffer gets a memset, and who accumulates).  EDVR tape; more backward launches than the
    default plan.
    Measured: worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; 218 backward launches, the default plan 203."""
    _run_child("fuse_res", default_arm)


@gpu
def test_fuse_res_bwd_0_fuse_act_bwd_0_edvr_tape(default_arm):
    """DVSR_FUSE_RES_BWD=0 DVSR_FUSE_ACT_BWD=0: the fully unfused backward.  EDVR tape; more backward launches than with either
    switch alone, each of which has more than the default plan.
    Measured: worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; 244 backward launches, 229 and 218 with one switch, the default plan 203."""
    _run_child("unfused", default_arm)


@gpu
def test_bwd_fork_every_1_bwd_probe_0_edvr_and_estimator_tapes(default_arm):
    """DVSR_BWD_FORK_EVERY=1 DVSR_BWD_PROBE=0: a side-stream fork per layer, on the shared, unprobed side stream.  EDVR tape and
    the estimator tape at (1,5,12,12); dvsr_switch_value is the proof (launches move between streams, no arithmetic changes).
    Measured: EDVR worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; estimator output 8.2e-7 of 1e-5, worst parameter gradient 2.2e-6 of 2e-4."""
    _run_child("fork_probe", default_arm)


@gpu
def test_tsa_dual_0_tsa_v_1_up2_4(default_arm):
    """DVSR_TSA_DUAL=0 DVSR_TSA_V=1 DVSR_UP2=4: fea_fusion and sAtt_1 as two 1x1 launches (the dual / fused_into wiring), the
    scalar TSA gate kernel (tsa_gate_fwd_kernel) and upsample2x_fwd_kernel, four input columns per thread.  EDVR tape, whose
    output is not bit-equal to the default arm's; test_tsa_gate_and_blend and test_upsample_bilinear of test_gpu_ops.
    Measured: EDVR worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; the worst rel-L2 of test_tsa_gate_and_blend 2.7e-7 of 1e-6, of test_upsample_bilinear 1.5e-7 of 1e-6."""
    _run_child("tsa_up2", default_arm)


@gpu
def test_tsa_v_4(default_arm):
    """DVSR_TSA_V=4: tsa_gate_fwd_vec_kernel<4> where HW % 4 == 0, the scalar kernel elsewhere (HW = 35, 18).
    test_tsa_gate_and_blend of test_gpu_ops at its bars (1e-6; measured: worst 2.7e-7 over the four cases)."""
    _run_child("tsa_v4", default_arm)


@gpu
def test_wgrad_split3_0_edvr_and_estimator_tapes(default_arm):
    """DVSR_WGRAD_SPLIT3=0: the plans ask for fp32 weight gradients.  EDVR tape and the estimator tape; the rule still answers a
    split kernel in mode 2 (the switch changes what the plans ask for), the EDVR plan issues nothing of its backward to the
    bf16 pipe, and some weight gradient is not bit-equal to the default arm's.
    Measured: EDVR worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4; estimator outputs 9.4e-7 of 1e-5, worst parameter gradient 3.3e-6 of 2e-4."""
    _run_child("wgrad_fp32", default_arm)


@gpu
def test_wgrad_wide_0_ops_and_edvr_tape(default_arm):
    """DVSR_WGRAD_WIDE=0: scalar staging in the fp32 and the split weight-gradient kernels (vector_width() == 0 in the three
    kernels it selects).  test_conv2d_backward and test_conv3x3_wgrad_split3 of test_gpu_ops, EDVR tape; the geometry query
    reports vx = 0 (and the scalar-staging split kernel) for a layer that has vx = 4 by default.
    Measured: the worst rel-L2 of test_conv2d_backward 7.5e-7 of 2e-5, of test_conv3x3_wgrad_split3 2.9e-7 of 2e-6; EDVR worst parameter gradient 1.8e-5 of 1e-4, input gradient 4.3e-5 of 5e-4."""
    _run_child("wgrad_scalar", default_arm)


@gpu
def test_est_fuse_pad_0_estimator_tape(default_arm):
    """DVSR_EST_FUSE_PAD=0: the estimators' reflection pads as separate launches (pad_fwd_kernel in the forward, the
    gmask_padded = 0 forms of pad_bwd*_kernel).  The estimator tape; dvsr_switch_value is the proof.
    Measured: outputs 9.4e-7 of 1e-5, worst parameter gradient 3.3e-6 of 2e-4."""
    _run_child("est_pads", default_arm)


@gpu
def test_split_th8_from_1(default_arm):
    """DVSR_SPLIT_TH8_FROM=1: 8-row tiles of the split conv kernel at every size (by default from 200 workgroups on, which no
    bf16_mfma = 2 test of the suite reaches below the large estimator shapes).  test_edvr_backward_all_grads_vs_oracle[2] and
    test_edvr_split_bf16_mfma_path of test_gpu_edvr; dvsr_switch_value is the proof.
    Measured: gradients: median rel-L2 3.3e-3 against the CPU fp32 oracle's 1.9e-3, worst 6.0e-3 of 2e-2; output 9.9e-7 of 2e-5, residual branch 1.9e-6 (the same figures as with 4-row tiles)."""
    _run_child("th8", default_arm)
