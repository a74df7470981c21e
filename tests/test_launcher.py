"""``python -m relevance_factorizationmachine_amd.run`` runs a driver as
``python SCRIPT ARGS`` would, with the reference's module names of this path bound to this
package.  Every case runs a child process against a decoy reference tree (launcher_common.py),
from a current directory outside that tree, with this repository on PYTHONPATH: the setting in
which a plain ``python driver.py`` binds the decoy (``test_plain_run_binds_the_decoy``).  No GPU."""
import json
import os

import pytest

from launcher_common import DECOY, RAN, ROOT, child_env, launch, python, ran, write_tree

TIMEOUT = 120
ENV = child_env(ROOT)
ARGS = ["setting=kuairec", "--x=1", "-m", "not.a.module"]  # (all of them the driver's)

DRIVER = RAN + '''\
import json
import os
import sys

torch = sys.modules.get("torch")
gpu_initialised = torch is not None and torch.cuda.is_initialized()
if "--exit=3" in sys.argv:
    sys.exit(3)
if "--raise" in sys.argv:
    raise RuntimeError("the decoy driver failed")

from src.fm import FactorizationMachines as FM
from src.mf import LogisticMatrixFactorization as MF
from src.base import PointwiseBaseRecommender
from utils.optimizer import SGD, BaseOptimizer
import src.extra
import utils.evaluate

import relevance_factorizationmachine_amd as pkg

print("REPORT", json.dumps({
    "ours": {"FM": FM is pkg.FactorizationMachines, "MF": MF is pkg.LogisticMatrixFactorization,
             "PointwiseBaseRecommender": PointwiseBaseRecommender is pkg.PointwiseBaseRecommender,
             "SGD": SGD is pkg.DeviceSGD},
    "decoys": sorted(c.__name__ for c in (FM, MF, PointwiseBaseRecommender, SGD, BaseOptimizer)
                     if getattr(c, "decoy", False)),
    "evaluate": utils.evaluate.__file__, "extra": src.extra.__file__,
    "argv": sys.argv, "name": __name__, "file": __file__, "path0": sys.path[0], "cwd": os.getcwd(),
    "gpu_initialised": gpu_initialised,
}))
'''
ALL_OURS = {"FM": True, "MF": True, "PointwiseBaseRecommender": True, "SGD": True}


@pytest.fixture
def tree(tmp_path):
    """(decoy reference root, its driver, a current directory outside the tree)"""
    ref = write_tree(tmp_path / "reference", {**DECOY, "driver.py": DRIVER})
    cwd = tmp_path / "elsewhere"
    cwd.mkdir()
    return ref, os.path.join(ref, "driver.py"), str(cwd)


def report(result) -> dict:
    assert result.returncode == 0, result.stderr
    lines = [line for line in result.stdout.splitlines() if line.startswith("REPORT ")]
    assert len(lines) == 1, result.stdout + result.stderr
    return json.loads(lines[0][len("REPORT "):])


def assert_bound(rep, ref):
    """This package's classes under the reference's names; every other module is the tree's."""
    assert rep["ours"] == ALL_OURS, rep
    assert rep["decoys"] == ["BaseOptimizer"], rep  # the rest of utils/optimizer.py is the reference's
    assert os.path.samefile(rep["evaluate"], os.path.join(ref, "utils", "evaluate.py"))
    assert os.path.samefile(rep["extra"], os.path.join(ref, "src", "extra.py"))
    assert rep["gpu_initialised"] is False


def test_script_form(tree):
    ref, driver, cwd = tree
    rep = report(launch([os.path.relpath(driver, cwd), *ARGS], cwd, ENV, TIMEOUT))
    assert_bound(rep, ref)
    assert rep["argv"][1:] == ARGS and os.path.samefile(rep["argv"][0], driver)
    assert rep["name"] == "__main__" and os.path.isabs(rep["file"]) and os.path.samefile(rep["file"], driver)
    assert os.path.samefile(rep["path0"], ref) and os.path.samefile(rep["cwd"], cwd)
    # the tree's src/fm.py, src/mf.py and src/base.py never ran; its optimizer.py ran for BaseOptimizer
    assert ran(ref) == {"driver.py", "src/extra.py", "utils/evaluate.py", "utils/optimizer.py"}


def test_plain_run_binds_the_decoy(tree):
    """The control: PYTHONPATH puts this repository ahead of the reference, but ``python SCRIPT``
    puts the script's directory ahead of PYTHONPATH, so the drivers' imports find the reference."""
    ref, driver, cwd = tree
    rep = report(python([driver, *ARGS], cwd, child_env(ROOT, ref), TIMEOUT))
    assert not any(rep["ours"].values()), rep
    assert rep["decoys"] == ["BaseOptimizer", "FactorizationMachines", "LogisticMatrixFactorization",
                             "PointwiseBaseRecommender", "SGD"]


def test_module_form(tree):
    ref, driver, cwd = tree
    rep = report(launch(["--reference", ref, "-m", "driver", *ARGS], cwd, ENV, TIMEOUT))
    assert_bound(rep, ref)
    assert rep["argv"][1:] == ARGS and os.path.samefile(rep["argv"][0], driver)
    assert rep["name"] == "__main__" and os.path.samefile(rep["file"], driver)
    assert os.path.samefile(rep["path0"], ref) and os.path.samefile(rep["cwd"], cwd)


def test_exit_status_passes_through(tree):
    ref, driver, cwd = tree
    result = launch([driver, "--exit=3"], cwd, ENV, TIMEOUT)
    assert result.returncode == 3, result.stderr


def test_uncaught_exception_fails_with_its_traceback(tree):
    ref, driver, cwd = tree
    result = launch([driver, "--raise"], cwd, ENV, TIMEOUT)
    assert result.returncode != 0
    assert "Traceback" in result.stderr and f'File "{driver}"' in result.stderr, result.stderr
    assert "RuntimeError: the decoy driver failed" in result.stderr


def test_check_reports_the_binding_and_runs_nothing(tree):
    ref, driver, cwd = tree
    result = launch(["--check", driver, "setting=kuairec"], cwd, ENV, TIMEOUT)
    assert result.returncode == 0, result.stderr
    where = dict(line.split(None, 1) for line in result.stdout.splitlines() if line.strip())
    for name, module in (("src.fm.FactorizationMachines", "fm"), ("src.mf.LogisticMatrixFactorization", "mf"),
                         ("src.base.PointwiseBaseRecommender", "base"), ("utils.optimizer.SGD", "optimizer")):
        assert where[name].startswith(f"relevance_factorizationmachine_amd.{module}."), where
        assert os.path.join(ROOT, "relevance_factorizationmachine_amd", module + ".py") in where[name], where
    assert os.path.samefile(where["utils.evaluate"], os.path.join(ref, "utils", "evaluate.py"))
    assert ran(ref) == set()  # neither the driver nor any module of the tree


OWN_OPTIMIZER = {
    "imports": "from . import optimizer  # noqa: F401\n",
    "installs": ("import importlib.util\nimport os\nimport sys\n\n"
                 "spec = importlib.util.spec_from_file_location(\n"
                 "    'utils.optimizer', os.path.join(os.path.dirname(__file__), 'optimizer.py'))\n"
                 "optimizer = importlib.util.module_from_spec(spec)\n"
                 "spec.loader.exec_module(optimizer)\n"
                 "sys.modules['utils.optimizer'] = optimizer\n"),
}


@pytest.mark.parametrize("init", list(OWN_OPTIMIZER.values()), ids=list(OWN_OPTIMIZER))
def test_reference_utils_with_its_own_optimizer(tree, init):
    """A reference ``utils/__init__.py`` that imports (or puts in place) its own ``optimizer``:
    the driver gets DeviceSGD, or the launcher stops before the driver and names the module."""
    ref, driver, cwd = tree
    write_tree(ref, {"utils/__init__.py": init})
    result = launch([driver], cwd, ENV, TIMEOUT)
    if result.returncode == 0:
        rep = report(result)
        assert rep["ours"] == ALL_OURS and "SGD" not in rep["decoys"], rep
    else:
        assert "utils.optimizer" in result.stderr, result.stderr
        assert "driver.py" not in ran(ref)


def test_tree_without_the_reference_packages_is_refused(tree, tmp_path):
    ref, driver, cwd = tree
    empty = tmp_path / "empty"
    empty.mkdir()
    result = launch(["--reference", str(empty), driver], cwd, ENV, TIMEOUT)
    assert result.returncode != 0 and "--reference" in result.stderr, result.stderr
    assert "driver.py" not in ran(ref)
