"""The switch table of the fp32 epoch launch (csrc/kernels/mlp_persistent_f32.hip, ``g_sw``): every
``mlp_set_*`` entry point reaches its own row, and every ``mlp_f32_*_last`` exists. No kernel is launched.
"""

import pytest

from _mlp_f32_fit import SWITCHES, lib  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def test_every_switch_has_its_own_override(lib):
    """`set` returns the override it replaces: -1 (none), then 0, then 1, switch by switch. While one
    switch is held at 0 or 1, setting it must not have moved any other: each of the others still
    answers -1 to a `set(-1)`. And every `mlp_f32_*_last` answers with an int."""
    setters = [getattr(lib, name) for name in SWITCHES]
    assert len(setters) == 7
    try:
        for s in setters:
            s(-1)
        for i, s in enumerate(setters):
            assert s(0) == -1, SWITCHES[i]
            assert s(1) == 0, SWITCHES[i]
            for j, other in enumerate(setters):
                if j != i:
                    assert other(-1) == -1, f"{SWITCHES[i]} moved {SWITCHES[j]}"
            assert s(-1) == 1, SWITCHES[i]
            assert s(-1) == -1, SWITCHES[i]
    finally:
        for s in setters:
            s(-1)
    for name in SWITCHES[1:]:  # (the plain-publish switch has none: mlp_debug_plain_seen)
        last = getattr(lib, name.replace("mlp_set_f32_", "mlp_f32_") + "_last")()
        assert isinstance(last, int) and last in (-1, 0, 1), (name, last)
