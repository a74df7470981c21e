"""Run one of the reference's drivers, unchanged, on this package::

    python -m relevance_factorizationmachine_amd.run [--reference DIR] [--check] SCRIPT [ARGS...]
    python -m relevance_factorizationmachine_amd.run [--reference DIR] [--check] -m MODULE [ARGS...]

``python main_kuairec.py`` puts the script's own directory at ``sys.path[0]``, ahead of every
``PYTHONPATH`` entry, so the driver's ``from src.fm import FactorizationMachines`` finds the
reference's ``src/fm.py`` whatever ``PYTHONPATH`` says.  This launcher binds the reference's
module names of this path (``BINDINGS``) to this package in ``sys.modules`` before any of the
driver's code runs, then runs the driver as ``python SCRIPT ARGS`` / ``python -m MODULE ARGS``
would: ``sys.argv[1:]`` is ARGS, ``sys.path[0]`` is the script's directory (the reference root
for ``-m``), the driver runs as ``__main__`` with ``__file__`` set, the current directory is
left alone and the exit status passes through.

The reference root (``--reference DIR``; by default the script's directory, or the current
directory for ``-m``) supplies the packages ``src`` and ``utils``: every module of theirs other
than the bound ones -- ``utils.evaluate``, ``utils.dataloader.*``, ``utils.search_params``, any
other ``src.*`` -- is the reference's own file.  A bound module holds this package's object
under the reference's name; any other name asked of it (``utils.optimizer.BaseOptimizer``) comes
from the reference's own file of that module, which runs in the bound module the first time such
a name is asked for.  If, after the reference's ``src/__init__.py`` and ``utils/__init__.py``
have run, a bound name no longer resolves to this package, the launcher exits non-zero before
the driver starts.  ``--check`` does the binding, prints where every bound name and
``utils.evaluate`` resolve, and exits without running the driver.

The launcher does not touch the GPU, change the environment or replace the process.  Under
``torch.distributed.run`` it is the module every worker runs
(``--nproc-per-node N -m relevance_factorizationmachine_amd.run main_kuairec.py ...``).
"""
from __future__ import annotations

import importlib.util
import os
import runpy
import sys
import types
from importlib.machinery import SourceFileLoader
from typing import Dict, List, Optional, Tuple

from . import DeviceSGD, FactorizationMachines, LogisticMatrixFactorization, PointwiseBaseRecommender

PROG = "relevance_factorizationmachine_amd.run"
USAGE = (f"usage: python -m {PROG} [--reference DIR] [--check] SCRIPT [ARGS...]\n"
         f"       python -m {PROG} [--reference DIR] [--check] -m MODULE [ARGS...]")

# the reference's module -> {name in it: this package's object}
BINDINGS: Dict[str, Dict[str, object]] = {
    "src.base": {"PointwiseBaseRecommender": PointwiseBaseRecommender},
    "src.fm": {"FactorizationMachines": FactorizationMachines},
    "src.mf": {"LogisticMatrixFactorization": LogisticMatrixFactorization},
    "utils.optimizer": {"SGD": DeviceSGD},
}
PACKAGES = ("src", "utils")


class LaunchError(Exception):
    """The reference cannot be bound as asked; none of the driver's code has run."""


class BoundModule(types.ModuleType):
    """One of the reference's modules bound to this package (an entry of ``BINDINGS``)."""

    def __init__(self, name: str, objects: Dict[str, object], reference_file: str):
        super().__init__(name, f"{name} bound to {__package__} by {PROG}")
        self.__dict__.update(objects)
        self._rfm_objects = objects
        self._rfm_reference_file = reference_file

    def __getattr__(self, attr: str):
        # any other name: the reference's own file of this module, run here once
        path = None if attr.startswith("__") else self.__dict__.pop("_rfm_reference_file", None)
        if path is None or not os.path.isfile(path):
            raise AttributeError(f"module {self.__name__!r} has no attribute {attr!r}")
        self.__file__ = path
        SourceFileLoader(self.__name__, path).exec_module(self)
        self.__dict__.update(self._rfm_objects)
        return getattr(self, attr)


def bind(reference: str) -> Dict[str, BoundModule]:
    """Import the reference's ``src`` and ``utils`` packages from ``reference`` under their own
    names, with the modules of ``BINDINGS`` in ``sys.modules`` (and as attributes of their
    package) before either package's ``__init__.py`` runs.  Returns the bound modules."""
    root = os.path.abspath(reference)
    packages = []
    for name in PACKAGES:
        init = os.path.join(root, name, "__init__.py")
        if not os.path.isfile(init):
            raise LaunchError(f"{init} not found: give the reference's root with --reference DIR")
        spec = importlib.util.spec_from_file_location(name, init,
                                                      submodule_search_locations=[os.path.dirname(init)])
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        packages.append(module)
    bound = {}
    for name, objects in BINDINGS.items():
        package, _, leaf = name.rpartition(".")
        bound[name] = BoundModule(name, objects, os.path.join(root, package, leaf + ".py"))
        sys.modules[name] = bound[name]
        setattr(sys.modules[package], leaf, bound[name])
    for module in packages:
        module.__spec__.loader.exec_module(module)
    return bound


def verify(bound: Dict[str, BoundModule]) -> None:
    """Raise ``LaunchError`` naming the module when a name of ``BINDINGS`` no longer resolves to
    this package (the reference's ``utils/__init__.py`` put its own ``optimizer`` in place, say)."""
    for name, objects in BINDINGS.items():
        module = sys.modules.get(name)
        package, _, leaf = name.rpartition(".")
        if (module is not bound[name] or getattr(sys.modules.get(package), leaf, None) is not module
                or any(module.__dict__.get(k) is not v for k, v in objects.items())):
            raise LaunchError(f"{name} is not bound to {__package__} after the reference's packages were "
                              f"imported (it is {module!r}); the driver was not run")


def report(reference: str, target: str) -> None:
    """``--check``: where every bound name and ``utils.evaluate`` resolve, one per line."""
    lines = [("reference", os.path.abspath(reference))]
    for name, objects in BINDINGS.items():
        for attr in objects:
            obj = getattr(sys.modules[name], attr)
            where = getattr(sys.modules.get(obj.__module__), "__file__", None)
            lines.append((f"{name}.{attr}", f"{obj.__module__}.{obj.__qualname__} ({where})"))
    spec = importlib.util.find_spec("utils.evaluate")
    lines.append(("utils.evaluate", spec.origin if spec is not None else "NOT FOUND"))
    lines.append(("driver", f"{target} (not run: --check)"))
    width = max(len(key) for key, _ in lines)
    for key, value in lines:
        print(f"{key:<{width}}  {value}")


def usage_error(message: str) -> SystemExit:
    print(f"{USAGE}\n{PROG}: error: {message}", file=sys.stderr)
    return SystemExit(2)


def parse(argv: List[str]) -> Tuple[Optional[str], bool, Optional[str], Optional[str], List[str]]:
    """``(reference, check, script, module, driver args)``: the launcher's options come first;
    everything after SCRIPT or ``-m MODULE`` belongs to the driver."""
    reference, check, i = None, False, 0
    while i < len(argv):
        arg = argv[i]
        if arg == "--check":
            check, i = True, i + 1
        elif arg in ("--reference", "-m"):
            if i + 1 == len(argv):
                raise usage_error(f"{arg} needs an argument")
            if arg == "-m":
                return reference, check, None, argv[i + 1], argv[i + 2:]
            reference, i = argv[i + 1], i + 2
        elif arg.startswith("--reference="):
            reference, i = arg.partition("=")[2], i + 1
        elif arg in ("-h", "--help"):
            print(USAGE)
            raise SystemExit(0)
        elif arg.startswith("-"):
            raise usage_error(f"unknown option {arg!r} (the launcher's options go before SCRIPT)")
        else:
            return reference, check, arg, None, argv[i + 1:]
    raise usage_error("no SCRIPT or -m MODULE")


def main(argv: Optional[List[str]] = None) -> None:
    reference, check, script, module, args = parse(sys.argv[1:] if argv is None else argv)
    if script is not None:
        target = os.path.abspath(script)  # (``python SCRIPT`` makes ``__file__`` absolute too)
        if not os.path.isfile(target):
            print(f"{PROG}: can't open file {target!r}", file=sys.stderr)
            raise SystemExit(2)
        path0 = os.path.dirname(os.path.realpath(target))
        reference = path0 if reference is None else reference
    else:
        target = f"-m {module}"
        reference = os.getcwd() if reference is None else reference
        path0 = os.path.abspath(reference)
    sys.path[0] = path0  # (in place of the current directory ``python -m`` put there)
    try:
        verify(bind(reference))
    except LaunchError as e:
        print(f"{PROG}: {e}", file=sys.stderr)
        raise SystemExit(1) from None
    if check:
        report(reference, target)
    elif script is not None:
        sys.argv = [target, *args]
        runpy.run_path(target, run_name="__main__")
    else:
        sys.argv = [module, *args]  # (run_module puts the module's file in sys.argv[0])
        runpy.run_module(module, run_name="__main__", alter_sys=True)


if __name__ == "__main__":
    main()
