"""Opt-in: route the reference's own ``training.train.rollout_test`` to the fused engine.

The drop-in replaces only the reference's ``models`` package.  With it,
the reference's ``rollout_test`` (training/train.py:67-95) steps the model in Python and
every step is one HIP ``msw_forward``.  ``install_fused_rollout()`` swaps that function for
:func:`mswegnn.rollout.rollout_test` (same semantics, the whole T-step loop as ONE
``msw_rollout``) inside the reference's module, so ``LightningTrainer.validation_step`` /
``predict_step`` (train.py:157-185), which look the name up in their module's globals at
call time, reach the fused path with no change to the callers.  ``models/__init__.py``
calls it when ``MSWEGNN_FUSED_ROLLOUT=1``.  The reference's function stays available as
``training.train._reference_rollout_test``.

``install_fused_loss()`` does the same for the name ``loss_function`` in ``training.train``
(bound there by ``from training.loss import loss_function``; ``training_step``,
train.py:125-145, looks it up at call time): it becomes :func:`mswegnn.loss.loss_function`,
the HIP loss kernels on a GPU and an op-for-op torch composition elsewhere.
``MSWEGNN_FUSED_LOSS=1`` installs it; the original stays as
``training.train._reference_loss_function``.
"""
import importlib.abc
import sys

TARGET = "training.train"


WANTED = set()  # "rollout", "loss": what the installed hooks replace


def _patch(mod):
    if "rollout" in WANTED:
        from .rollout import rollout_test
        if getattr(mod, "rollout_test", None) is not rollout_test:
            mod._reference_rollout_test = getattr(mod, "rollout_test", None)
            mod.rollout_test = rollout_test
    if "loss" in WANTED:
        from .loss import loss_function
        if getattr(mod, "loss_function", None) is not loss_function:
            mod._reference_loss_function = getattr(mod, "loss_function", None)
            mod.loss_function = loss_function


class _PatchingLoader(importlib.abc.Loader):
    def __init__(self, loader):
        self.loader = loader

    def create_module(self, spec):
        return self.loader.create_module(spec)

    def exec_module(self, module):
        self.loader.exec_module(module)
        _patch(module)


class _Finder(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path, target=None):
        if name != TARGET:
            return None
        for f in sys.meta_path:
            if f is self or not hasattr(f, "find_spec"):
                continue
            spec = f.find_spec(name, path, target)
            if spec is not None:
                if spec.loader is not None:
                    spec.loader = _PatchingLoader(spec.loader)
                return spec
        return None


PENDING = False  # training.train was mid-import when the hook was installed


def _initializing(mod):
    return bool(getattr(getattr(mod, "__spec__", None), "_initializing", False))


def install_fused_rollout():
    """Patch ``training.train.rollout_test`` now if it is imported, else when it is.

    If ``training.train`` is itself being imported (it imports ``models`` through
    utils.miscellaneous before defining ``rollout_test``), the patch is applied by
    :func:`maybe_patch` at the first model call instead."""
    _install("rollout")


def install_fused_loss():
    """Patch ``training.train.loss_function`` -- the name ``from training.loss import
    loss_function`` bound there, which ``training_step`` looks up at call time -- with
    :func:`mswegnn.loss.loss_function`, now if ``training.train`` is imported, else when it is
    (mid-import: at the first model call, as for the rollout)."""
    _install("loss")


def _install(what):
    global PENDING
    WANTED.add(what)
    mod = sys.modules.get(TARGET)
    if mod is not None:
        if _initializing(mod):
            PENDING = True
        else:
            _patch(mod)
    if not any(isinstance(f, _Finder) for f in sys.meta_path):
        sys.meta_path.insert(0, _Finder())


def maybe_patch():
    global PENDING
    mod = sys.modules.get(TARGET)
    if mod is not None and not _initializing(mod):
        _patch(mod)
        PENDING = False
