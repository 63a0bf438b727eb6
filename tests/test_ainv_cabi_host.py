"""CPU tests (-m "not gpu") of cmi_plan_set_row_scale: the exported symbol with its prototype and Python wrapper, its declaration (no stream: it
launches nothing), and the refusal that happens before any device call (on a machine without a GPU anything that reached the device would come
back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

INVALID = 1


def test_symbol_prototype_and_wrapper(cmi):
    L = cmi.lib()
    assert L.cmi_plan_set_row_scale.argtypes is not None and len(L.cmi_plan_set_row_scale.argtypes) == 2
    assert callable(cmi.plan_set_row_scale) and cmi.binding.plan_set_row_scale is cmi.plan_set_row_scale


def test_declaration_takes_a_plan_and_an_array_and_no_stream():
    text = open(os.path.join(ROOT, "include", "cusp_mi355x.h")).read()
    m = re.search(r"int\s+cmi_plan_set_row_scale\s*\(([^)]*)\)\s*;", text)
    assert m, "cmi_plan_set_row_scale is not declared in include/cusp_mi355x.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["cmi_plan *plan", "const void *scale_dev"]


def test_null_plan_is_refused_without_a_device_call(cmi):
    L = cmi.lib()
    buf = (ctypes.c_char * 4096)()
    for scale in (None, ctypes.addressof(buf)):
        assert L.cmi_plan_set_row_scale(None, scale) == INVALID
        assert b"null plan" in L.cmi_last_error(), L.cmi_last_error()
    with pytest.raises(cmi.CmiError) as e:
        cmi.plan_set_row_scale(None, None)
    assert e.value.status == INVALID
