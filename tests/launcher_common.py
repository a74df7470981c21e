"""A decoy reference tree for the tests of ``python -m relevance_factorizationmachine_amd.run``
(test_launcher.py, test_gpu_launcher.py): the reference's package, module and class names and
nothing else of it.  Every decoy class is marked ``decoy = True``, and every decoy module other
than a package's ``__init__.py`` leaves ``<its file>.ran`` behind when it runs, so a test can tell
which objects a driver was given and which of the tree's files were executed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAN = "open(__file__ + '.ran', 'w').close()\n"

DECOY = {
    "src/__init__.py": "",
    "src/base.py": RAN + "\n\nclass PointwiseBaseRecommender:\n    decoy = True\n",
    "src/fm.py": RAN + "from src.base import PointwiseBaseRecommender\n\n\n"
                       "class FactorizationMachines(PointwiseBaseRecommender):\n    decoy = True\n",
    "src/mf.py": RAN + "from src.base import PointwiseBaseRecommender\n\n\n"
                       "class LogisticMatrixFactorization(PointwiseBaseRecommender):\n    decoy = True\n",
    "src/extra.py": RAN,
    "utils/__init__.py": "",
    "utils/optimizer.py": RAN + "\n\nclass BaseOptimizer:\n    decoy = True\n\n\n"
                                "class SGD(BaseOptimizer):\n    decoy = True\n",
    "utils/evaluate.py": RAN + "\n\nclass ValEvaluator:\n    decoy = True\n",
}


def write_tree(root, files) -> str:
    """Write ``{relative path: text}`` under ``root``; returns ``root`` as a string."""
    for rel, text in files.items():
        path = os.path.join(str(root), rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return str(root)


def ran(tree) -> set:
    """The decoy files (relative paths) that were executed."""
    return {os.path.relpath(os.path.join(d, f), str(tree))[: -len(".ran")]
            for d, _, files in os.walk(str(tree)) for f in files if f.endswith(".ran")}


def child_env(*paths) -> dict:
    """This process's environment with ``paths`` in front of ``PYTHONPATH``."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([*paths, *filter(None, [env.get("PYTHONPATH")])])
    return env


def python(args, cwd, env, timeout):
    """``python ARGS`` in a child process (with ``-s`` when this one ignores the user's site)."""
    flags = ["-s"] if sys.flags.no_user_site else []
    return subprocess.run([sys.executable, *flags, *args], cwd=str(cwd), env=env, capture_output=True,
                          text=True, timeout=timeout)


def launch(args, cwd, env, timeout):
    """``python -m relevance_factorizationmachine_amd.run ARGS`` in a child process."""
    return python(["-m", "relevance_factorizationmachine_amd.run", *args], cwd, env, timeout)
