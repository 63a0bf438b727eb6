"""Plan creation's decision table on an MI355X: for every matrix and request of tools/plan_routes.py the plan's status (and error text), its
whole config, info(), device_bytes() and shifted_tiles() equal tests/golden/plan_routes.json, which was recorded once at the commit it names.
A refactor of csrc/plan.hip passes this unmodified; the golden file is re-recorded only by a change that means to alter a rule.  Nothing is
multiplied here: the bit-exact checks of every kernel are the other modules'.

Each environment switch is read once per process, so each setting's rows come from a child process of its own with a time limit; after a
child that was killed, timed out or died of a signal no further case of this module touches the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_routes as pr  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "plan_routes.json")) as _f:
    GOLDEN = json.load(_f)

_stopped = []  # why the module stopped using the GPU (a child that faulted or hung)

# every route the table must show: (kernel of the resulting plan, was a kernel asked for?)
AUTO_ROUTES = {"CSR_STREAM", "CSR_BALANCED", "CSR_STREAM_C16", "CSR_STREAM_WAVE", "CSR_STREAM_WAVEV", "CSR_STREAM_WAVEX", "CSR_STREAM_WAVER", "COO_LANE4", "COO_TILE"}
ASKED_ROUTES = {"CSR_SCALAR", "CSR_VECTOR", "CSR_STREAM", "CSR_STREAM_PIPE", "CSR_STREAM_C16", "CSR_STREAM_WAVE", "CSR_STREAM_WAVEV", "CSR_STREAM_WAVEX", "CSR_STREAM_WAVER",
                "CSR_STREAM_PACKED", "COO_TILE"}


def _compare(got, want, where):
    assert set(got) == set(want), (where, sorted(set(got) ^ set(want)))
    for label in want:
        assert got[label] == want[label], (where, label, got[label], want[label])


def test_table_covers_every_route(cmi):
    """The golden table has the tool's matrices, requests and settings -- all of them -- and between them every route: a trimmed table fails."""
    assert len(GOLDEN["recorded_at_commit"]) == 40
    assert set(GOLDEN["matrices"]) == set(pr.MATRICES) and set(GOLDEN["environment"]) == set(pr.ENV_SETTINGS)
    seen, errors = set(), set()
    for name, rows in GOLDEN["matrices"].items():
        assert set(rows) == {pr.label(r) for r in pr.requests_of(name)}, name
        for lab, row in rows.items():
            if row["status"]:
                errors.add(row["error"].split(": ", 1)[1][:60])
            else:
                seen.add((row["config"]["kernel"], "kernel=" in lab))
    for setting, per_matrix in GOLDEN["environment"].items():
        assert set(per_matrix) == set(pr.ENV_SETTINGS[setting]), setting
        for name, rows in per_matrix.items():
            assert set(rows) == {pr.label(r) for r in pr.env_requests(setting, name)}, (setting, name)
            seen |= {(row["config"]["kernel"], False) for row in rows.values() if not row["status"]}
    assert seen == {(getattr(cmi, k), False) for k in AUTO_ROUTES} | {(getattr(cmi, k), True) for k in ASKED_ROUTES}
    # the two "asked for but not possible" errors, the partition's, the constructors' refusals and the row offsets' check
    for text in ("cmi_plan_create: CMI_CSR_STREAM_WAVER / _PACKED need f64 values", "cmi_plan_create: CMI_CSR_STREAM_WAVEV needs items_per_thread",
                 "cmi_plan_create: wave tiles on a row partition need", "cmi_plan_create: CMI_CSR_STREAM_WAVER needs the column indices",
                 "cmi_plan_create_csr: CMI_CSR_STREAM_PACKED copies the values", "cmi_plan_create: CMI_CSR_STREAM_C16 needs the column indices",
                 "cmi_plan_create: row offsets run from", "cmi_plan_create: CMI_COO_TILE needs row-sorted entries"):
        assert any(e.startswith(text[:60]) for e in errors), text
    # the only way into the plan-built csr_wave for AUTO plans; each switch changes at least one of its rows
    wave2 = GOLDEN["environment"]["CMI_CSR_WAVE=2"]["irregular"]["plan:f64"]["config"]
    assert wave2["kernel"] == cmi.CSR_STREAM_WAVE and wave2["rows_per_block"] == 0
    for setting, per_matrix in GOLDEN["environment"].items():
        assert any(rows[lab] != GOLDEN["matrices"][name].get(lab) for name, rows in per_matrix.items() for lab in rows), setting


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pr.MATRICES))
def test_routes_of_matrix(cmi, name):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert not _stopped, _stopped
    _compare(pr.run_matrix(name), GOLDEN["matrices"][name], name)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(pr.ENV_SETTINGS))
def test_routes_under_environment_switch(cmi, setting):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    assert not _stopped, _stopped
    try:
        got = pr.run_env_child(setting, timeout=300)
    except (subprocess.TimeoutExpired, pr.ChildDied) as e:
        _stopped.append(f"{setting}: {e}")
        raise
    for name, rows in GOLDEN["environment"][setting].items():
        _compare(got[name], rows, (setting, name))
