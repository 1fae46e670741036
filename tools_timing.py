"""What the tools_*_timing.py scripts and tools_refit_quality.py share: the statistics of a series, the two ways of timing a
call (wall clock, HIP events on the call's stream), a child process per library or under `rocprofv3 --kernel-trace`, and the
JSON document at the end.  What a script measures, and every constant it measures with, is in that script."""
import contextlib
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time


def repo_on_path():
    """raytracing_folder_amd and tests are imported from the tree the scripts lie in"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def add_common_args(ap, calls=200):
    """--calls (unless None), --width, --height, --out"""
    if calls is not None:
        ap.add_argument("--calls", type=int, default=calls)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)


def spread(values, digits=4):
    values = sorted(values)
    return dict(median=round(statistics.median(values), digits), min=round(values[0], digits), max=round(values[-1], digits), n=len(values))


def timed(fn, calls, warmup):
    """the spread of the wall time, in ms, of fn(i) for i in warmup .. warmup + calls - 1, after fn(0) .. fn(warmup - 1)"""
    out = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn(i)
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def event_times(stream, calls, n, warmup=10, batch=1):
    """{name: [ms, ...]} for the callables of `calls`, which enqueue on `stream` (a torch.cuda.Stream): `warmup` rounds of every
    call and a stream synchronisation, then `n` rounds, the calls interleaved in dict order; in a round each call -- `batch` of it
    back to back -- lies between two HIP events on the stream, and the second is waited for before the next call starts"""
    import torch
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            for c in calls.values():
                c()
        stream.synchronize()
        for _ in range(n):
            for k, c in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(batch):
                    c()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    return ms


def _child(cmd, env, timeout, what):
    """a fresh child process; one that died says why, and nothing more is started on the device"""
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return r


@contextlib.contextmanager
def kernel_trace_db(script, child_args, env=None, prefix="trace_", timeout=600):
    """`rocprofv3 --kernel-trace -d DIR -o trace -- python script child_args` as a child process; yields an open sqlite3 connection
    to the trace's database (its `kernels` view: kernel_durations_us) and removes DIR afterwards"""
    tmp = tempfile.mkdtemp(prefix=prefix)
    try:
        _child(["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(script), *map(str, child_args)],
               env, timeout, "kernel trace (%s)" % " ".join(map(str, child_args)))
        dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
        if not dbs:
            raise SystemExit("kernel trace: rocprofv3 left no database")
        with contextlib.closing(sqlite3.connect(dbs[0])) as db:
            yield db
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_durations_us(db, kernel, where=""):
    """the durations, in start order, of the dispatches whose kernel name holds `kernel` (`where`: more SQL conditions, " and ...")"""
    return [row[0] / 1000.0 for row in db.execute(f"select end - start from kernels where name like '%{kernel}%'{where} order by start")]


def per_library(script, libs_arg, child_args, each=None):
    """--libs name=path,...: {name: the document of `python script child_args` run as a child with RT_MI355X_LIB=path} (the last
    line of its stdout); each(name, env, document), if given, runs after a library's child, with the child's environment"""
    res = {}
    for item in libs_arg.split(","):
        name, path = item.split("=", 1)
        env = dict(os.environ, RT_MI355X_LIB=os.path.abspath(path))
        r = _child([sys.executable, os.path.abspath(script), *map(str, child_args)], env, 600, name)
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        if each:
            each(name, env, res[name])
    return res


def emit(res, out):
    """the document as one line on stdout and, indented, in the file `out` (if given)"""
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
