"""CPU checks around BUIR: the float64 restatement the GPU tests compare against equals float64 torch autograd of the reference
formula typed again; the model's initial state is bit-identical to the reference's under the same seed; the torch-path model
reproduces the reference's loss, gradients, full_predict scores and two five-step Adam runs with the target update (g13); the
optimizer property fires the target update once per step; eval_factors() scores equal full_predict's; the tolerances stand above
the fp32 floor of the stock path and deliberately wrong variants land above them; the new entry points refuse bad arguments
before any launch."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buir_ref as R  # noqa: E402
from whisprrec_amd import host  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_buir.npz")


@pytest.fixture(scope="module")
def g13():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return [R.make_case(i) for i in range(len(R.CASES))]


@pytest.fixture(scope="module")
def refs(cases):
    return [R.buir_f64(c) for c in cases]


@pytest.fixture(scope="module")
def runs64(g13):
    """the float64 runs (a) and (b) from g13's initial state"""
    sd = _sd(g13)
    return {tag: R.adam_run(sd, g13["users"], g13["items"], m, lr) for tag, (m, lr) in R.RUNS.items()}


def _sd(g13):
    return {str(n): g13["sd__" + str(n)] for n in g13["names"]}


def _args(**kw):
    base = dict(device="cpu", model_path="/tmp/wr_buir.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64, momentum=0.995,
                buir_native=0)
    base.update(kw)
    return argparse.Namespace(**base)


def _model(g13=None, **kw):
    from whisprrec_amd.buir import BUIR
    m = BUIR(_args(**kw), host.Corpus(R.N_USERS, R.N_ITEMS, {}))
    if g13 is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(g13).items()})
    return m


def _feed(g13):
    return {"user_id": torch.from_numpy(g13["users"]), "pos_item": torch.from_numpy(g13["items"]),
            "neg_items": torch.ones(len(g13["users"]), 1, dtype=torch.int64), "batch_size": len(g13["users"]), "phase": "train"}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_restatement_equals_the_reference_formula_in_float64_under_autograd(cases, refs, i):
    got = R.stock_torch(cases[i], dtype=torch.float64)
    fig = R.figures(got, refs[i])
    fig["dU"], fig["dI"] = R.rel_err(got["dU"], refs[i]["dU"]), R.rel_err(got["dI"], refs[i]["dI"])
    assert max(fig.values()) <= 1e-12, fig


def test_zero_target_row_has_term_two_and_no_gradient(cases, refs):
    i = [c[0] for c in R.CASES].index("zero_target")
    c, ref = cases[i], refs[i]
    k = 0                                                # sample 0's item target row is zero: its user-side term is 2
    xi = c["Io"][c["items"][k]].astype(np.float64)
    p = c["W"].astype(np.float64) @ xi + c["b"]
    tu = c["Ut"][c["users"][k]].astype(np.float64)
    c_iu = (p / np.linalg.norm(p)) @ (tu / max(np.linalg.norm(tu), R.EPS))
    assert abs(ref["terms"][k] - (2.0 + 2.0 - 2.0 * c_iu)) < 1e-12
    assert np.abs(ref["gU"][k]).max() == 0.0


def test_ema_fp32_is_the_three_rounding_form_and_an_fma_is_not():
    rng = np.random.RandomState(5)
    t, o = rng.standard_normal((1000, 64)).astype(np.float32), rng.standard_normal((1000, 64)).astype(np.float32)
    for m in (0.995, 0.9, 0.0, 1.0):
        want = (torch.from_numpy(t) * m + torch.from_numpy(o) * (1. - m)).numpy()
        assert np.array_equal(R.ema_fp32(t, o, m), want), m
    m = 0.995
    fused = (np.float64(t) * np.float64(np.float32(m)) + np.float64(np.float32(o * np.float32(1. - m)))).astype(np.float32)
    assert (fused != R.ema_fp32(t, o, m)).sum() > 1000    # one rounding fewer is visible bitwise


# ------------------------------------------------------------------------------------------------ the model against g13
def test_g13_batch_is_as_described(g13):
    assert g13["users"].shape == g13["items"].shape == (96,)
    assert len(np.unique(g13["users"])) <= 8 and len(np.unique(g13["items"])) <= 12
    assert [str(n) for n in g13["names"]] == ["user_online.weight", "user_target.weight", "item_online.weight",
                                               "item_target.weight", "predictor.weight", "predictor.bias"]


def test_initial_state_is_the_references_bit_for_bit(g13):
    torch.manual_seed(3407)
    m = _model()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in g13["names"]]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g13["sd__" + k]), k
    assert np.array_equal(sd["user_target.weight"].numpy(), sd["user_online.weight"].numpy())
    assert not m.user_target.weight.requires_grad and not m.item_target.weight.requires_grad
    assert m.count_variables() == (R.N_USERS + R.N_ITEMS) * 64 + 64 * 64 + 64


def test_torch_path_reproduces_the_reference(g13):
    m = _model(g13)
    m.train()
    loss = m.predict(_feed(g13))
    loss.backward()
    ref = float(g13["loss"][0])
    assert abs(float(loss.detach()) - ref) <= R.LOSS_TOL * abs(ref)
    for n, p in m.named_parameters():
        if p.requires_grad:
            e = R.rel_err(p.grad.numpy(), g13["g__" + n])
            assert e <= R.TOL, (n, e)
        else:
            assert p.grad is None
    with torch.no_grad():
        scores = m.full_predict({"user_id": torch.from_numpy(g13["fp_users"])}).numpy()
    assert scores.shape == (4, R.N_ITEMS) and R.rel_err(scores, g13["fp_scores"]) <= R.TOL


def _model_run(g13, tag, steps=5, **kw):
    """five steps of the reference loop (zero_grad / predict / backward / step) through the optimizer property"""
    momentum, lr = R.RUNS[tag]
    m = _model(g13, momentum=momentum, **kw)
    m.train()
    m.optimizer = torch.optim.Adam(m.parameters(), lr=lr)
    curve = []
    for _ in range(steps):
        m.optimizer.zero_grad()
        loss = m.predict(_feed(g13))
        loss.backward()
        m.optimizer.step()
        curve.append(float(loss.detach()))
    return np.asarray(curve), {k: v.numpy().copy() for k, v in m.state_dict().items() if k in R.TABLES}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_torch_path_adam_runs_reproduce_the_reference(g13, tag):
    curve, tables = _model_run(g13, tag)
    gt = {k: g13[tag + "_sd__" + k] for k in R.TABLES}
    fig = R.run_figures(curve, tables, _sd(g13), g13[tag + "_losses"].astype(np.float64), gt)
    print(R.run_fmt(tag, fig))
    assert fig["losses"] <= R.RUN_TOL["losses"] and fig["online_update"] <= R.RUN_TOL["online_update"], fig
    if tag == "b":                                       # run (a)'s target move is below what fp32 can judge (buir_ref)
        assert fig["target_update"] <= R.RUN_TOL["target_update"], fig
    untouched = np.setdiff1d(np.arange(R.N_USERS), g13["users"])
    assert len(untouched) == 42
    assert np.array_equal(tables["user_target.weight"][untouched], gt["user_target.weight"][untouched])


# ------------------------------------------------------------------------------------------------ the optimizer hook
def test_optimizer_property_fires_the_target_update_once_per_step(g13):
    m = _model(g13)
    assert m.optimizer is None
    keys = list(m.state_dict().keys())
    calls = []
    real = m._update_target
    m._update_target = lambda: (calls.append(1), real())
    m.optimizer = torch.optim.SGD(m.parameters(), lr=0.1)
    assert list(m.state_dict().keys()) == keys and "optimizer" not in dict(m.named_modules())
    before = m.user_target.weight.detach().clone()
    for k in range(3):
        m.optimizer.zero_grad()
        m.predict(_feed(g13)).backward()
        m.optimizer.step()
        assert len(calls) == k + 1
    assert not torch.equal(before, m.user_target.weight.detach())
    old = m.optimizer
    m.optimizer = None                                   # as BaseModel.__init__ assigns it
    assert m.optimizer is None
    old.step()
    assert len(calls) == 3                               # the hook left with the optimizer
    m.optimizer = torch.optim.SGD(m.parameters(), lr=0.1)
    m.optimizer = torch.optim.SGD(m.parameters(), lr=0.1)
    m.optimizer.step()
    assert len(calls) == 4                               # re-assignment does not stack hooks


def test_model_trains_under_base_runner_fit():
    """BaseRunner.fit builds the optimizer itself; the target tables must follow without a runner of BUIR's own"""
    from whisprrec_amd.buir import BUIR
    from whisprrec_amd.runner import BaseRunner
    rng = np.random.RandomState(3)
    uu, ii = rng.randint(0, 20, 200), rng.randint(1, 30, 200)
    corpus = host.Corpus.from_arrays(20, 30, (uu, ii))
    torch.manual_seed(1)
    m = BUIR(_args(embedding_size=32), corpus)
    parser = BaseRunner.parse_runner_args(argparse.ArgumentParser())
    run = BaseRunner(parser.parse_args(["--batch_size", "64", "--lr", "0.01"]))
    before = m.item_target.weight.detach().clone()
    np.random.seed(1)
    loss = run.fit(BUIR.Dataset(m, corpus, "train"))
    assert np.isfinite(loss) and 0.0 < loss < 4.0
    assert not torch.equal(before, m.item_target.weight.detach())
    assert not torch.equal(m.item_target.weight.detach(), m.item_online.weight.detach())


# ------------------------------------------------------------------------------------------------ evaluation factors
def test_eval_factors_scores_equal_full_predict(g13):
    m = _model(g13)
    with torch.no_grad():
        users = torch.arange(R.N_USERS)
        want = m.full_predict({"user_id": users}).numpy().astype(np.float64)
    Uf, If = m.eval_factors()
    assert Uf.shape == (R.N_USERS, 128) and If.shape == (R.N_ITEMS, 128) and not Uf.requires_grad and not If.requires_grad
    got = (Uf @ If.t()).numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ tolerances and power
def test_tolerances_stand_above_the_fp32_floor(cases, refs, g13, runs64):
    worst = {k: 0.0 for k in R.FIGS}
    for i, c in enumerate(cases):
        fig = R.figures(R.stock_torch(c), refs[i])
        print(R.fmt("floor " + R.CASES[i][0], fig))
        for k in R.FIGS:
            worst[k] = max(worst[k], fig[k])
    assert max(worst.values()) * 4 < R.TOL, worst
    assert R.TOL <= 8 * max(R.FLOORS.values()) * 1.25                      # 8 x the floor, rounded up to one digit: no more
    sd = _sd(g13)
    for tag, (momentum, lr) in R.RUNS.items():
        l32, t32 = R.adam_run(sd, g13["users"], g13["items"], momentum, lr, dtype=torch.float32)
        fig = R.run_figures(l32, t32, sd, *runs64[tag])
        print(R.run_fmt("floor " + tag, fig))
        assert fig["losses"] * 4 < R.RUN_TOL["losses"] and fig["online_update"] * 4 < R.RUN_TOL["online_update"], fig
        if tag == "b":
            assert fig["target_update"] * 4 < R.RUN_TOL["target_update"], fig
        else:
            assert fig["target_update"] > 10 * R.RUN_TOL["target_update"]     # why run (a) cannot judge the target update
    for k in R.RUN_TOL:
        assert R.RUN_TOL[k] <= 8 * R.RUN_FLOORS[k] * 1.25


@pytest.mark.parametrize("wrong", R.WRONG)
def test_wrong_gradients_land_above_the_tolerance(cases, refs, wrong):
    for i, c in enumerate(cases):
        fig = R.figures(R.buir_f64(c, wrong=wrong), refs[i])
        assert max(fig.values()) > 100 * R.TOL, (R.CASES[i][0], fig)


@pytest.mark.parametrize("wrong", R.RUN_WRONG)
def test_wrong_target_updates_land_above_the_tolerance_on_run_b(g13, runs64, wrong):
    momentum, lr = R.RUNS["b"]
    sd = _sd(g13)
    lw, tw = R.adam_run(sd, g13["users"], g13["items"], momentum, lr, wrong=wrong)
    fig = R.run_figures(lw, tw, sd, *runs64["b"])
    assert fig["target_update"] > 100 * R.RUN_TOL["target_update"], fig
    for m in (0.995, 0.9):                               # and on the update alone, away from the fixed points m = 1/2, o = t
        t, o = sd["user_target.weight"] + 0.01, sd["user_online.weight"]
        good, bad = R.ema_f64(t, o, m), R.ema_f64(t, o, m, wrong=wrong)
        assert R.rel_err(bad - t, good - t) > 0.5


# ------------------------------------------------------------------------------------------------ interface
def _lib():
    from whisprrec_amd import abi
    assert os.path.exists(abi.LIB_PATH), "run __graft_entry__.build() first"    # a missing library is a failed build, not a skip
    return abi, abi.lib()


def test_launcher_knows_the_model_and_its_flags():
    from whisprrec_amd import main as launcher
    args, model_cls, reader_cls, runner_cls = launcher.build_args(["--model_name", "BUIR", "--buir_native", "1", "--momentum", "0.9"])
    assert model_cls.__name__ == "BUIR" and reader_cls.__name__ == "BaseReader" and runner_cls.__name__ == "BaseRunner"
    assert args.buir_native == 1 and args.momentum == 0.9 and args.embedding_size == 64
    assert "momentum=0.9" in args.log_file and "embedding_size=64" in args.log_file
    args = launcher.build_args(["--model_name", "BUIR"])[0]
    assert args.buir_native == 0 and args.momentum == 0.995


def test_supported_set_and_workspace():
    abi, L = _lib()
    assert [L.wr_buir_supported(D) for D in (32, 64, 128, 16, 48, 256)] == [1, 1, 1, 0, 0, 0]
    for D in (32, 64, 128):
        for B in (1, 128, 129, 2048, 65536):
            wgs = (B + 127) // 128
            assert L.wr_buir_workspace_bytes(B, D) >= wgs * (D * D + D + 1) * 4
    assert L.wr_buir_workspace_bytes(0, 64) == -2 and "B=0" in abi.last_error()
    assert L.wr_buir_workspace_bytes((1 << 22) + 1, 64) == -2
    assert L.wr_buir_workspace_bytes(64, 48) == -5 and "D=48" in abi.last_error()


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    abi, L = _lib()
    buf = (ctypes.c_float * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(Uo=a16, Io=a16, Ut=a16, It=a16, nu=10, ni=10, D=64, W=a16, b=a16, users=a16, items=a16, B=4, loss=a16, gU=a16, gI=a16,
             gW=a16, gb=a16, ws=a16, ws_bytes=1 << 40):
        return L.wr_buir_loss_grad(Uo, Io, Ut, It, nu, ni, D, W, b, users, items, B, loss, gU, gI, gW, gb, None, ws, ws_bytes, None)

    assert call(D=48) == -5 and "D=48" in abi.last_error()
    assert call(D=256) == -5
    assert call(B=0) == -2 and call(B=(1 << 22) + 1) == -2 and call(nu=0) == -2
    for name in ("Uo", "Io", "Ut", "It", "W", "b", "users", "items", "loss"):
        assert call(**{name: None}) == -1, name
    assert "NULL" in abi.last_error()
    assert call(gI=None) == -1 and call(gW=None) == -1 and call(gb=None) == -1
    assert call(Uo=a16 + 4) == -4 and call(W=a16 + 4) == -4 and call(gU=a16 + 4) == -4
    assert call(ws_bytes=1024) == -3 and call(ws=None) == -3 and "wr_buir_loss_grad" in abi.last_error()

    assert L.wr_ema_update(None, a16, 16, 0.9, 0.1, None) == -1 and L.wr_ema_update(a16, None, 16, 0.9, 0.1, None) == -1
    assert L.wr_ema_update(a16, a16, 0, 0.9, 0.1, None) == -2
    assert L.wr_ema_update(a16 + 4, a16, 16, 0.9, 0.1, None) == -4 and "wr_ema_update" in abi.last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from whisprrec_amd import abi, hip_ops
    U, I, W, b = torch.zeros(10, 64), torch.zeros(12, 64), torch.zeros(64, 64), torch.zeros(64)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.buir_loss_grad(U, I, U, I, W, b, ids, ids)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.buir_loss(U, I, U, I, W, b, ids, ids)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.ema_update_(U.clone(), U, 0.9)
    assert hip_ops.buir_supports(64) and not hip_ops.buir_supports(48)
    assert hip_ops.buir_workspace_bytes(129, 64) >= 2 * (64 * 64 + 64 + 1) * 4


def test_native_flag_on_an_unsupported_size_keeps_the_torch_path(g13, caplog):
    m = _model(embedding_size=48, buir_native=1)
    with caplog.at_level("WARNING"):
        loss = m.predict({"user_id": torch.from_numpy(g13["users"]), "pos_item": torch.from_numpy(g13["items"])})
        m._update_target()
    assert np.isfinite(float(loss.detach())) and m._buir_native_ok is False
    assert sum("buir_native" in r.getMessage() for r in caplog.records) == 1


# ------------------------------------------------------------------------------------------------ the drop-in stub
REF = "/root/reference"
BUIR_STUB = """from models.BaseModel import GeneralModel
from whisprrec_amd.buir import bind
BUIR = bind(GeneralModel)
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference tree not present on this machine")
def test_stub_replaces_the_references_file_and_trains_under_its_own_runner(tmp_path):
    """INTEGRATION.md's three lines in place of src/models/general/BUIR.py: the reference's main.py finds the class, chains its
    flags, builds it from its reader and trains an epoch on the CPU under its own BaseRunner (the torch path; no HIP call), then
    evaluates.  What follows the evaluation is the reference's own log formatting, which newer NumPy versions refuse."""
    import shutil
    import subprocess
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    shutil.copytree(os.path.join(REF, "src"), tmp_path / "src")
    shutil.copytree(os.path.join(REF, "data", "ml-100k"), tmp_path / "data" / "ml-100k")
    (tmp_path / "src" / "models" / "general" / "BUIR.py").write_text(BUIR_STUB)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "main.py", "--model_name", "BUIR", "--lr", "0.001", "--dataset", "ml-100k", "--path",
           str(tmp_path / "data") + "/", "--log_file", str(tmp_path / "log.txt"), "--model_path", str(tmp_path / "m.pt"),
           "--num_workers", "0", "--gpu", "", "--epoch", "1", "--batch_size", "2048"]
    res = subprocess.run(cmd, cwd=tmp_path / "src", env=env, capture_output=True, text=True, timeout=600)
    out = res.stdout + res.stderr
    assert "#params: 165248" in out                     # (943 + 1574) * 64 + 64 * 64 + 64: the targets are not counted
    assert "Optimizer: Adam" in out and "Predict" in out and "WhisprRecHipError" not in out
    assert res.returncode == 0 or "np.float_" in out, out[-2000:]
