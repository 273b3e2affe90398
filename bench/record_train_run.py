"""Record what one training run prints and writes, as a JSON digest: the tool for "a refactor of the training
application changed nothing".  Run it in a checkout of the parent commit and in the changed tree and diff the outputs.

    python bench/record_train_run.py --row cpu-main --set b --out digest.jsonl     # one run, one JSON line appended
    python bench/record_train_run.py --list cpu | gpu                              # the (row, set) pairs of a machine

A row is a flow and an engine: ``main_no_ddp.py`` (plain module / single device) or ``main.py`` at world size 1
(``FlatBucketDDP`` or the fused trainer), on the CPU with one thread (``--engine torch``), or on a GPU with ``--engine
fused`` in bf16 and fp32 and ``--engine ops``.  A set is a group of options on top of ``--synthetic 256 --batch-size 32
--epochs 2 --eval 64 --metrics-json``; the ``e_*`` sets run epoch 1, then ``--resume`` to epoch 2 (``main.py`` only:
``main_no_ddp.py`` writes no checkpoint).  Every run is a fresh child process in an empty working directory, which
seeds torch (the scripts do not: their initial weights differ from run to run) and then runs ``main_no_ddp.py`` as
``__main__`` or calls ``main.main(0, 1, cfg)``, the per-rank entry ``main.py`` spawns.

The digest holds: the stdout lines without the ``training time`` line; the metrics records without the timing fields;
every file written -- for ``*.pt`` files each entry's dtype, shape, sha256 of its bytes and alias group (entries that
share storage share a group), for ``*.meta.json`` the content.  Nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--synthetic", "256", "--batch-size", "32", "--epochs", "2", "--eval", "64", "--metrics-json", "metrics.json"]
_B = ["--momentum", "0.9", "--weight-decay", "5e-4", "--lr-schedule", "cosine", "--lr-warmup-steps", "2"]
_C = ["--optimizer", "adamw", "--weight-decay", "0.05", "--ema-decay", "0.9", "--ema-warmup"]
SETS = {"a": [], "b": _B, "c": _C, "d": _C + ["--augment"], "e_b": _B, "e_c": _C}
ENGINES = {"cpu": ["--engine", "torch"], "fused-bf16": ["--engine", "fused", "--dtype", "bf16"],
           "fused-fp32": ["--engine", "fused", "--dtype", "fp32"], "ops": ["--engine", "ops"]}
TIMING_FIELDS = ("seconds", "step_ms", "images_per_sec", "allreduce_us_per_step", "seconds_total", "time")
CKPT = os.path.join("ckpt", "birds_vs_airplanes.pt")


def rows(machine: str) -> list:
    engines = ["cpu"] if machine == "cpu" else [e for e in ENGINES if e != "cpu"]
    return [(f"{e}-{flow}", s) for e in engines for flow in ("no_ddp", "main") for s in SETS
            if flow == "main" or not s.startswith("e_")]


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def commands(row: str, opt_set: str) -> list:
    engine, flow = row.rsplit("-", 1)
    args = BASE + ENGINES[engine] + SETS[opt_set]
    child = [os.path.abspath(__file__), "--child", flow]
    if flow == "no_ddp":
        return [child + args]
    main = child + ["--backend", "gloo" if engine == "cpu" else "nccl", "--checkpoint-path", CKPT,
                    "--port", str(_free_port())]  # (several rows may run at the same time)
    if not opt_set.startswith("e_"):
        return [main + args]
    one = [a if a != "2" or args[i - 1] != "--epochs" else "1" for i, a in enumerate(args)]
    return [main + one, main + args + ["--resume", CKPT]]


def tensor_entries(obj, prefix: str = "", groups=None) -> dict:
    """{key path: digest} of a loaded ``*.pt`` object: nested dicts are flattened, other leaves kept as they are."""
    import torch
    groups = {} if groups is None else groups
    out = {}
    for k, v in obj.items():
        key = f"{prefix}{k}"
        if isinstance(v, dict):
            out.update(tensor_entries(v, key + "/", groups))
        elif isinstance(v, torch.Tensor):
            raw = v.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
            alias = groups.setdefault((v.untyped_storage().data_ptr(), v.storage_offset(), tuple(v.shape)), len(groups))
            out[key] = {"dtype": str(v.dtype), "shape": list(v.shape), "alias_group": alias,
                        "sha256": hashlib.sha256(raw).hexdigest()}
        else:
            out[key] = v
    return out


def digest_dir(work: str) -> dict:
    import torch
    files, metrics = {}, []
    for d, _, names in sorted(os.walk(work)):
        for name in sorted(names):
            path = os.path.join(d, name)
            rel = os.path.relpath(path, work)
            if rel == "metrics.json":
                with open(path) as f:
                    metrics = [{k: v for k, v in json.loads(ln).items() if k not in TIMING_FIELDS} for ln in f]
            elif name.endswith(".pt"):
                files[rel] = tensor_entries(torch.load(path, map_location="cpu", weights_only=True))
            elif name.endswith(".json"):
                with open(path) as f:
                    files[rel] = json.load(f)
            else:
                files[rel] = None  # a file nobody expected: the name alone
    return {"metrics": metrics, "files": files}


def child(flow: str, argv: list) -> None:
    """The run itself, in the child process."""
    import runpy

    import torch
    torch.manual_seed(0)
    if "torch" in argv:  # the CPU rows
        torch.set_num_threads(1)
    sys.path.insert(0, ROOT)
    sys.argv = [os.path.join(ROOT, "main_no_ddp.py")] + argv
    if flow == "no_ddp":
        runpy.run_path(sys.argv[0], run_name="__main__")
        return
    import main as M
    M.main(0, 1, M.config_from_args(M._parse(argv), M.data_path))


def record(row: str, opt_set: str, timeout: float) -> dict:
    env = dict(os.environ, PYTHONPATH=ROOT)
    stdout, codes = [], []
    with tempfile.TemporaryDirectory() as work:
        for cmd in commands(row, opt_set):
            res = subprocess.run([sys.executable] + cmd, cwd=work, env=env, capture_output=True, text=True,
                                 timeout=timeout)
            codes.append(res.returncode)
            stdout += [ln for ln in res.stdout.splitlines() if not ln.startswith("training time")]
            if res.returncode != 0:
                stdout += ["[stderr] " + ln for ln in res.stderr.splitlines()[-20:]]
                break
        return {"row": row, "set": opt_set, "returncodes": codes, "stdout": stdout, **digest_dir(work)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--list", choices=["cpu", "gpu"], help="print this machine's (row, set) pairs and exit")
    ap.add_argument("--row", help="<engine>-<flow>, e.g. cpu-main, fused-bf16-no_ddp, ops-main")
    ap.add_argument("--set", dest="opt_set", choices=sorted(SETS))
    ap.add_argument("--out", help="append the digest as one JSON line (default: print it)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
    ap.add_argument("--child", choices=["no_ddp", "main"], help=argparse.SUPPRESS)
    a, rest = ap.parse_known_args()
    if a.child:
        child(a.child, rest)
        return 0
    if a.list:
        for row, s in rows(a.list):
            print(row, s)
        return 0
    rec = record(a.row, a.opt_set, a.timeout)
    line = json.dumps(rec, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    else:
        print(line)
    return 0 if all(c == 0 for c in rec["returncodes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
