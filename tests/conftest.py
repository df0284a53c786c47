import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "dp2: two data-parallel ranks sharing cuda:0 (workers start at collection time)")
    config.addinivalue_line("markers", "bench_gpus2: `python bench.py --gpus 2` launched bare at collection time")


# ---- 2-rank data-parallel GPU tests ---------------------------------------------------------------------------------
# The rank processes are started by tests/dp_launcher.py, itself started HERE, right after collection and before any test has
# run, i.e. while this pytest process has not initialised the GPU yet (a GPU-initialised process must not fork+exec children).
# The launcher never touches the GPU; it keeps at most DP2_MAX_GPU_PROCS of its processes on the GPU at a time, so that the
# suite never holds more than DP2_MAX_GPU_PROCS + 1 GPU processes at once (a shared GPU machine caps that count).  The ranks
# run concurrently with the tests and write .npz dumps that tests/test_hip_dp2.py waits for and checks.
DP2 = {"jobs": {}, "dir": None, "launcher": None}
DP2_MAX_GPU_PROCS = 8


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def pytest_collection_finish(session):
    order = []                                           # cases in the order the tests ask for them
    for item in session.items:
        for m in item.iter_markers("dp2"):
            if m.args and m.args[0] not in order:
                order.append(m.args[0])
    want_bench = any(item.get_closest_marker("bench_gpus2") for item in session.items)
    if (not order and not want_bench) or session.config.option.collectonly:
        return
    import json
    import subprocess
    import tempfile
    DP2["dir"] = d = tempfile.mkdtemp(prefix="stem_dp2_")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    if torch.cuda.device_count() < 2:                    # counting devices does not initialise the GPU
        order = [c for c in order if not c.startswith("rccl2_")]      # two real RCCL ranks need a device each: those tests skip
    jobs = []
    for case in order:
        port = _free_port()
        world = 1 if case.startswith("rccl1_") else 2    # rccl1_*: ONE rank in a world-size-1 RCCL ("nccl") process group
        procs = [{"argv": [sys.executable, os.path.join(REPO, "tests", "dp_worker.py"), "--case", case, "--rank", str(r), "--world", str(world),
                           "--port", str(port), "--out", d],
                  "log": os.path.join(d, f"{case}_rank{r}.log"), "err": None, "rc": os.path.join(d, f"{case}_rank{r}.rc")} for r in range(world)]
        jobs.append({"name": case, "gpu_procs": world, "env": env, "procs": procs})

    # `python bench.py --gpus 2` typed bare on a one-GPU machine (the command form the driver uses): started the same way; its parent
    # starts the two ranks and never touches the GPU.  --full: the test checks the roofline figures of the run too.
    if want_bench:
        env_b = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
        env_b["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        env_b["STEM_BENCH_VERIFY"] = "1"
        jobs.append({"name": "bench2", "gpu_procs": 2, "env": env_b, "procs": [
            {"argv": [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"],
             "log": os.path.join(d, "bench2.out"), "err": os.path.join(d, "bench2.err"), "rc": os.path.join(d, "bench2.rc")}]})
    for job in jobs:
        DP2["jobs"][job["name"]] = [p["rc"] for p in job["procs"]]
    with open(os.path.join(d, "jobs.json"), "w") as f:
        json.dump(jobs, f)
    DP2["launcher"] = subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "dp_launcher.py"), "--jobs", os.path.join(d, "jobs.json"),
                                        "--max-procs", str(DP2_MAX_GPU_PROCS), "--parent", str(os.getpid())], stdout=open(os.path.join(d, "launcher.log"), "w"),
                                       stderr=subprocess.STDOUT)


def pytest_sessionfinish(session, exitstatus):
    launcher = DP2.get("launcher")
    if launcher is not None and launcher.poll() is None:
        launcher.terminate()                             # kills the jobs it started
        try:
            launcher.wait(timeout=30)
        except Exception:
            launcher.kill()


def dp2_wait(name, timeout=900):
    """exit statuses of the processes of job `name` (a dp2 case or "bench2"), waiting for them; "timeout" for a process that ran
    longer than `timeout` seconds (it is killed, with its children: the launcher then starts nothing more), the launcher's
    "not started: <why>" for a job it did not start.  Time spent queued behind other jobs does not count."""
    import time
    from dp_launcher import kill_tree
    rcs = DP2["jobs"].get(name)
    assert rcs, f"dp2 job {name!r} was not started (collection hook)"
    out = []
    for rc in rcs:
        while not os.path.exists(rc):
            if os.path.exists(rc + ".pid") and time.time() - os.path.getmtime(rc + ".pid") > timeout:
                try:
                    kill_tree(int(open(rc + ".pid").read()))
                except ValueError:
                    pass
                out.append("timeout")
                break
            if DP2["launcher"].poll() is not None and not os.path.exists(rc):
                log = open(os.path.join(DP2["dir"], "launcher.log")).read()[-2000:]
                pytest.fail(f"dp2 launcher exited with {DP2['launcher'].returncode} before job {name} finished:\n{log}")
            time.sleep(0.5)
        else:
            text = open(rc).read()
            out.append(int(text) if text.lstrip("-").isdigit() else text)
    return out


@pytest.fixture(scope="session")
def dp2_results():
    """wait(case) -> [rank0 dump, rank1 dump] (dicts of numpy arrays); fails with the worker logs if a rank died."""
    def wait(case, timeout=900):
        for r, rc in enumerate(dp2_wait(case, timeout)):
            if rc != 0:
                log = open(os.path.join(DP2["dir"], f"{case}_rank{r}.log")).read()[-4000:]
                pytest.fail(f"dp2 worker {case} rank {r} exited with {rc}:\n{log}")
        return [dict(np.load(os.path.join(DP2["dir"], f"{case}_rank{r}.npz"))) for r in range(len(DP2["jobs"][case]))]
    return wait


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))
        return cache[name]

    return load


def close_ratio(a, b, floor, atol=0.0):
    """max over elements of (|a - b| - atol) / max(|b|, floor * max|b|): the quantity assert_close bounds by rtol."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()), 1e-30)
    return float((np.maximum(np.abs(a - b) - atol, 0.0) / np.maximum(np.abs(b), floor * scale)).max())


def assert_close(a, b, rtol=1e-4, atol=0.0, what="", *, floor):
    """north_star tolerance: 1e-4 relative (fp32).  `atol` is stated per call site where the quantity has a natural
    absolute floor (e.g. likelihoods are floored at 1e-9).  `floor` is stated per call site too: fp32 summation error is
    relative to the magnitude of the summed terms, not of a cancelling result, so elements smaller than `floor` x max|b|
    are held to the absolute bound rtol x floor x max|b| (floor=0.1 -> 1e-5 of the tensor's maximum, about ten times the
    fp32 noise of the dot products on this path; floor=0 is a pure element-wise relative test)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    scale = max(float(np.abs(b).max()), 1e-30)
    err = np.abs(a - b)
    tol = atol + rtol * np.maximum(np.abs(b), floor * scale)
    bad = err > tol
    assert not bad.any(), (f"{what}: {bad.sum()}/{bad.size} out of tolerance; max err {err.max():.3e} "
                           f"(scale {scale:.3e}) at {np.unravel_index(err.argmax(), err.shape)}")


def f64_gate(ours, exact, ref32_err, what, rtol=1e-4, atol=0.0, floor=0.1):
    """Parity gate against the float64 run of the reference (tests/golden/stem_f64.npz, make_golden.py:gen_f64): the HIP
    result must be within `rtol` (north_star: 1e-4) of the EXACT value; the reference's own fp32 error in the same
    metric is printed next to ours (it is the yardstick: e.g. torch's fp32 clip_grad_norm_ is ~1e-4 off the exact norm,
    so two correct fp32 implementations can legitimately sit 2e-4 apart)."""
    r = close_ratio(ours, exact, floor, atol)
    print(f"[f64 gate] {what}: HIP vs exact {r:.2e}   reference-fp32 vs exact {float(np.max(ref32_err)):.2e}   bound {rtol:.0e}")
    assert r <= rtol, f"{what}: HIP path is {r:.3e} from the float64 reference (bound {rtol:.0e}; the reference's own fp32 run: {float(np.max(ref32_err)):.3e})"
    return r
