"""CPU (no GPU needed): the block V-cycle's entry points exist in every layer and refuse the host mode
(tests/test_gpu_multigrid_block.py holds what they compute)."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["psp_mg_precon_block", "psp_mg_precon_block_dev", "psp_mg_block_reserve", "psp_mg_block_info"]


def test_new_symbols_are_declared_and_exported():
    from pysparse_amd import _capi
    L = _capi.lib()
    with open(os.path.join(ROOT, "include", "pysparse_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(L, name) and ("int %s(" % name) in header, name


def test_python_layers_have_the_methods():
    from pysparse_amd import device as dev
    from pysparse.precon import precon
    assert list(inspect.signature(dev.DeviceMultigrid.precon_block).parameters) == ["self", "X", "Y"]
    assert list(inspect.signature(dev.DeviceMultigrid.precon_block_dev).parameters) == ["self", "k", "x_ptr", "ldx", "y_ptr", "ldy"]
    assert callable(dev.DeviceMultigrid.block_info) and callable(dev.DeviceMultigrid.block_reserve)
    assert hasattr(precon.MultigridType, "precon_block")


def test_host_mode_has_no_block_cycle():
    """PSP_DEVICE=cpu: PSP_ENODEV (-2) from every entry point that would run kernels, before any argument is looked at"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from pysparse_amd import _capi\n"
            "L = _capi.lib()\n"
            "print('rc', L.psp_mg_precon_block(None, 2, None, 1, None, 1), L.psp_mg_precon_block_dev(None, 2, None, 1, None, 1),\n"
            "      L.psp_mg_block_reserve(None, 2))\n"
            "print(L.psp_last_error().decode())\n") % ROOT
    env = dict(os.environ)
    env["PSP_DEVICE"] = "cpu"
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "rc -2 -2 -2" in p.stdout and "PSP_DEVICE=cpu" in p.stdout, p.stdout
