"""One launcher for the CPU tests that look at a ``train_ddp.Solver``-built model: the routing switches are read when the Solver is
built and the layer modules' STATS count per process, so every setting gets a fresh child process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRELUDE = "import sys, torch\nsys.path[:0] = [%(root)r, %(pkg)r]\n"


def run_solver_script(body, cfg_name, env=None, device="cpu", text=False, timeout=900, **fmt):
    """Run ``body`` (python source that builds a Solver and prints one ``RESULT <int> ...`` line; ``%(cfg)r`` is the path of
    experiments/cfgs/``cfg_name``, ``%(device)r`` the device, ``%(name)r`` any further keyword) in a child process whose environment
    is this one's with ``env`` laid over it -- a value of None removes the variable.  -> the integers of the last RESULT line; with
    ``text`` also the child's standard output."""
    child = dict(os.environ)
    for k, v in (env or {}).items():
        child.pop(k, None)
        if v is not None:
            child[k] = v
    code = (_PRELUDE + body) % dict(fmt, root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"), device=device,
                                    cfg=os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    out = subprocess.run([sys.executable, "-c", code], env=child, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    ints = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    return (ints, out.stdout) if text else ints
