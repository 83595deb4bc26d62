"""Argument checks of gnnmp_stick_steer: they come before any device work (no GPU needed), and they are the ones
tests/test_abi_errors.py shows for the 2-D entry gnnmp_maze_steer."""
import ctypes

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_ARG = -1, -6


def test_stick_steer_argument_checks():
    L = _lib.lib()
    assert L.gnnmp_stick_steer(1, 4, 15, None, None, None, None, None, None, None, None, None) == ERR_NULL
    fake = ctypes.c_void_p(4096)
    # a missing status array is a null pointer like the others
    assert L.gnnmp_stick_steer(1, 4, 15, fake, fake, fake, fake, fake, fake, fake, None, None) == ERR_NULL
    assert L.gnnmp_stick_steer(0, 4, 15, fake, fake, fake, fake, fake, fake, fake, fake, None) == ERR_ARG
    assert L.gnnmp_stick_steer(1, 4, 0, fake, fake, fake, fake, fake, fake, fake, fake, None) == ERR_ARG
    assert L.gnnmp_stick_steer(1, -1, 15, fake, fake, fake, fake, fake, fake, fake, fake, None) == ERR_ARG
    # the steered path may not alias its inputs (null stream argument: the check comes before the launch)
    assert L.gnnmp_stick_steer(1, 4, 15, fake, fake, fake, fake, fake, fake, fake, fake, None) == ERR_ARG
    # waypoints without their arrays
    assert L.gnnmp_stick_steer(1, 4, 15, fake, fake, None, fake, fake, fake, fake, fake, None) == ERR_NULL
