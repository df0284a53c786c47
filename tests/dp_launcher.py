#!/usr/bin/env python3
"""Starts the processes of the 2-rank GPU tests (tests/conftest.py) a few at a time.  NOT a pytest module; never touches the GPU.

    python tests/dp_launcher.py --jobs DIR/jobs.json --max-procs N --parent PID

jobs.json is a list of {"name", "gpu_procs", "env", "procs": [{"argv", "log", "err", "rc"}]}.  The processes of one job start
together (the ranks of a process group rendezvous with each other) and only while the GPU processes of the running jobs and
the job's own stay within --max-procs; jobs start in list order.  As a process starts its pid goes to "<rc>.pid", as it ends its
exit status goes to "rc".

Nothing more is started once anything went wrong:
  * a process that exits non-zero stops the queue: its peers in the job are killed, and every job not yet started gets
    "not started: ..." as the content of its rc files (and in its logs), so that the tests waiting for it fail at once;
  * a process that ends by a signal (a GPU fault's abort, a segmentation fault, dp2_wait's kill after its time limit) or with
    124 / 134 / 137 / 139 also kills the jobs still running;
  * when the parent (pytest) is gone -- SIGTERM from the kernel (PR_SET_PDEATHSIG) or a changed parent pid -- or on SIGTERM,
    the running jobs are killed and the launcher exits.
The processes stay in the caller's process group (a group kill reaches them and their own children); every direct child also
gets SIGKILL should the launcher die first.
"""
import argparse
import ctypes
import json
import os
import signal
import subprocess
import sys
import time

PR_SET_PDEATHSIG = 1
FAULT_CODES = (124, 134, 137, 139)


def _pdeathsig(sig):
    try:
        ctypes.CDLL(None, use_errno=True).prctl(PR_SET_PDEATHSIG, int(sig), 0, 0, 0)
    except (OSError, AttributeError):
        pass


def descendants(pid):
    """pids of every process below `pid` (children first found through /proc/*/stat's parent field)"""
    parent = {}
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                with open(f"/proc/{d}/stat") as f:
                    parent[int(d)] = int(f.read().rsplit(")", 1)[1].split()[1])
            except (OSError, ValueError, IndexError):
                pass
    found, todo = [], [pid]
    while todo:
        p = todo.pop()
        kids = [c for c, pp in parent.items() if pp == p]
        found += kids
        todo += kids
    return found


def kill_tree(pid, killed=None):
    """SIGKILL `pid` and everything below it (`killed`: a set that records `pid`)"""
    if killed is not None:
        killed.add(pid)
    for p in [pid] + descendants(pid):
        try:
            os.kill(p, signal.SIGKILL)
        except OSError:
            pass


def _write(path, text):
    with open(path + ".tmp", "w") as f:
        f.write(text)
    os.replace(path + ".tmp", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", required=True)
    ap.add_argument("--max-procs", type=int, required=True)
    ap.add_argument("--parent", type=int, required=True, help="pid of the process that started the launcher")
    args = ap.parse_args()
    pending = json.load(open(args.jobs))
    running = []                       # (job, [(Popen, rc path)])
    killed = set()                     # pids this launcher killed itself: their ends are not a new failure

    def kill_running():
        for _, procs in running:
            for p, _ in procs:
                if p.poll() is None:
                    kill_tree(p.pid, killed)

    def stop(*_):
        kill_running()
        sys.exit(1)
    signal.signal(signal.SIGTERM, stop)
    _pdeathsig(signal.SIGTERM)
    if os.getppid() != args.parent:    # the parent died before the line above
        stop()

    def child_setup():
        _pdeathsig(signal.SIGKILL)

    stopped = None                     # why nothing more is started
    while pending or running:
        if os.getppid() != args.parent:
            stop()
        for entry in list(running):
            job, procs = entry
            for p, rc in procs:
                if p.poll() is not None and not os.path.exists(rc):
                    _write(rc, str(p.returncode))
                    if p.returncode != 0 and p.pid not in killed:
                        if stopped is None:
                            stopped = f"job {job['name']} (pid {p.pid}) exited with {p.returncode}"
                        print(f"dp_launcher: job {job['name']} (pid {p.pid}) exited with {p.returncode}; starting nothing more",
                              file=sys.stderr, flush=True)
                        if p.returncode < 0 or p.returncode in FAULT_CODES:
                            kill_running()
                        for q, _ in procs:     # its peers would wait for it in a collective until their time limit
                            if q.poll() is None:
                                kill_tree(q.pid, killed)
            if all(p.poll() is not None for p, _ in procs):
                running.remove(entry)
        if stopped is not None:
            for job in pending:
                for spec in job["procs"]:
                    for path in filter(None, (spec["log"], spec.get("err"))):
                        _write(path, f"not started: {stopped}\n")
                    _write(spec["rc"], f"not started: {stopped}")
            pending = []
        busy = sum(job["gpu_procs"] for job, _ in running)
        while pending and (not running or busy + pending[0]["gpu_procs"] <= args.max_procs):
            job = pending.pop(0)
            procs = []
            for spec in job["procs"]:
                out = open(spec["log"], "w")
                err = open(spec["err"], "w") if spec.get("err") else subprocess.STDOUT
                p = subprocess.Popen(spec["argv"], env=job["env"], stdout=out, stderr=err, preexec_fn=child_setup)
                _write(spec["rc"] + ".pid", str(p.pid))
                procs.append((p, spec["rc"]))
            running.append((job, procs))
            busy += job["gpu_procs"]
        time.sleep(0.2)


if __name__ == "__main__":
    main()
