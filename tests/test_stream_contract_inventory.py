"""The stream-contract table (tests/stream_contract.py) is complete: every family of include/cusp_mi355x.h that takes a `void *stream`
is in it exactly once, in one class, and every family whose stream behaviour is tested has a builder for each value type the header
declares.  A new entry point fails here until it has a row -- and with the row, a case in tests/test_stream_contract_gpu.py.  No GPU."""
import collections
import os

import stream_contract as SC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cusp_mi355x.h")


def declared():
    with open(HEADER) as f:
        return SC.header_families(f.read())


def test_the_parser_sees_the_header():
    """Comments are stripped first (a doc block that names `void *stream` declares nothing); typed families fold into one."""
    text = """/* int cmi_in_a_comment_f64(void *stream); */
    int cmi_one_f64(int64_t n, const double *x,
                    void *stream);
    int cmi_one_f32(int64_t n, const float *x, void *stream);  // int cmi_in_a_line_comment(void *stream);
    int cmi_no_stream(int64_t n);
    int cmi_untyped(const int32_t *Ap, void * stream);"""
    assert SC.header_families(text) == {"cmi_one": ["f64", "f32"], "cmi_untyped": [""]}
    families = declared()
    assert len(families) >= 126 and sum(map(len, families.values())) >= 216
    assert families["cmi_spmv_csr"] == ["f64", "f32"] and families["cmi_gather"] == ["i32", "f32", "f64"] and families["cmi_plan_create"] == [""]


def test_every_family_is_in_the_table_exactly_once():
    families = declared()
    count = collections.Counter(r.family for r in SC.ROWS)
    assert not [f for f, c in count.items() if c != 1], "a family has more than one row"
    missing = sorted(set(families) - set(count))
    assert not missing, f"entry points that take a stream and have no row in tests/stream_contract.py: {missing}"
    stale = sorted(set(count) - set(families))
    assert not stale, f"rows for families the header no longer declares: {stale}"
    assert all(r.cls in (SC.ASYNC, SC.SYNC, SC.OUT) for r in SC.ROWS)


def test_out_of_scope_is_the_agreed_list_and_says_why():
    out = [r for r in SC.ROWS if r.cls == SC.OUT]
    assert {r.family for r in out} <= set(SC.OUT_OF_SCOPE)
    assert set(SC.OUT_OF_SCOPE) == {
        "cmi_allgather", "cmi_allgatherv", "cmi_allreduce", "cmi_halo_exchange", "cmi_comm_barrier", "cmi_comm_allgather_host", "cmi_copy_ranges",
        "cmi_memcpy_h2d", "cmi_memcpy_d2h", "cmi_memcpy_d2d", "cmi_memcpy_d2h_async", "cmi_memset", "cmi_event_record", "cmi_stream_destroy",
        "cmi_stream_synchronize", "cmi_stream_wait_event"}
    assert all(r.reason and r.builder is None for r in out)


def test_every_tested_family_has_a_builder_for_each_declared_type():
    families = declared()
    for r in SC.ROWS:
        assert sorted(r.types) == sorted(families[r.family]), f"{r.family}: the row lists {r.types}, the header declares {families[r.family]}"
        if r.cls != SC.OUT:
            assert callable(r.builder), f"{r.family}: no builder"
    # the parametrisation of the GPU module is this table: one case per family and value type
    assert len(SC.cases(SC.ASYNC)) + len(SC.cases(SC.SYNC)) == sum(len(r.types) for r in SC.ROWS if r.cls != SC.OUT)
