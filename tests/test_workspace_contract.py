"""The workspace contract on the host (no device needed: the size queries are host functions): every size query the header
declares is in the case table of tests/workspace_cases.py or exempt for a stated reason, every query refuses the bad
arguments its header comment names, and every shape of the table still exercises the layout it was chosen for. The GPU
side is tests/test_workspace_contract_train_gpu.py and tests/test_workspace_contract_gpu.py."""
import pytest

import workspace_cases as wc

ALLOWED_EXEMPT = {
    "ossid_ppf_sample_workspace_bytes", "ossid_ppf_vote_workspace_bytes", "ossid_mesh_vertex_normals_workspace_bytes",
    "ossid_pn2_train_bn_stats_workspace_bytes", "ossid_conv3x3_c1_wgrad_workspace_bytes", "ossid_seg_bce_iou_workspace_bytes",
    "ossid_conv3x3_wgrad_workspace_bytes",
}
ALL_CASES = wc.TRAIN_CASES + wc.POSE_CASES


def _table():
    table = {}
    for case in ALL_CASES:
        for q in case.queries:
            assert q not in table, "%s is covered twice (%s, %s)" % (q, table[q].name, case.name)
            table[q] = case
    return table


def test_every_size_query_is_in_the_table_or_exempt_for_a_reason(hiplib):
    queries = [s for s in hiplib.exported_symbols() if s.endswith(wc.SUFFIXES)]
    assert len(queries) >= 37
    table = _table()
    assert set(wc.EXEMPT) <= ALLOWED_EXEMPT and all(isinstance(r, str) and r for r in wc.EXEMPT.values())
    assert not set(wc.EXEMPT) & set(table)
    missing = [q for q in queries if q not in table and q not in wc.EXEMPT]
    assert not missing, "size queries with no contract case: %s" % missing
    stale = [q for q in list(table) + list(wc.EXEMPT) if q not in queries]
    assert not stale, "the table names queries the header does not declare: %s" % stale


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_queries_refuse_the_bad_arguments_their_header_names(hiplib, case):
    for query, call in case.refusals:
        assert query in case.queries
        got = call(hiplib)
        for v in (got.values() if isinstance(got, dict) else [got]):
            assert int(v) <= 0, (query, v)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_every_shape_still_exercises_its_layout(hiplib, case):
    """The predicate of each shape, and per family one buffer whose size is no multiple of 512 bytes (the caching allocator's
    rounding then cannot swallow an overrun) unless the case says why no shape can have one."""
    assert case.shapes
    ragged = False
    for shape in case.shapes:
        need = case.need(hiplib, shape)
        assert set(need) == set(case.queries) and all(v > 0 for v in need.values()), (shape, need)
        case.predicate(hiplib, shape)
        sizes = case.nbytes(hiplib, shape)
        print(case.name, shape, need, "bytes", sizes, "not a multiple of 512:", [n for n in sizes if n % 512])
        ragged = ragged or any(n % 512 for n in sizes)
    assert ragged or not case.ragged, "%s: every queried size is a multiple of 512 bytes" % case.name
