"""index.search_route: which library entry, workspace function and pipelining chunk a search takes. A pure function of
(usable coarse copy, width, the wide_768 flag, query count) - no device, no library."""
import itertools

import pytest

QS = (1, 64, 65, 1024, 1025, 2200)
COARSE_WS = "clipmi_topk_ip_coarse_workspace_bytes"


@pytest.fixture(scope="module")
def route(clipmi):
    return clipmi.index.search_route


@pytest.mark.parametrize("d, wide_768, Q", itertools.product((512, 768), (False, True), QS))
def test_no_usable_coarse_copy_is_the_exact_search(route, d, wide_768, Q):
    r = route(None, d, wide_768, Q)
    assert r == ("clipmi_topk_ip", "clipmi_topk_ip_workspace_bytes", None)
    assert (r.entry, r.workspace, r.chunk) == tuple(r)


@pytest.mark.parametrize("d, wide_768, Q", itertools.product((512, 768), (False, True), QS))
def test_bf16_is_the_64_query_pass(route, d, wide_768, Q):
    assert route("bf16", d, wide_768, Q) == ("clipmi_topk_ip_coarse", COARSE_WS, 64)


@pytest.mark.parametrize("wide_768, Q", itertools.product((False, True), QS))
def test_int8_at_512_is_wide_inside_the_library(route, wide_768, Q):
    assert route("int8", 512, wide_768, Q) == ("clipmi_topk_ip_coarse_i8", COARSE_WS, 1024)


@pytest.mark.parametrize("Q", QS)
def test_int8_at_768_by_default_is_the_64_query_pass(route, Q):
    assert route("int8", 768, False, Q) == ("clipmi_topk_ip_coarse_i8", COARSE_WS, 64)


@pytest.mark.parametrize("Q", QS)
def test_int8_at_768_with_the_wide_pass(route, Q):
    r = route("int8", 768, True, Q)
    if Q <= 64:
        assert (r.entry, r.workspace) == ("clipmi_topk_ip_coarse_i8", COARSE_WS)
    else:
        assert r == ("clipmi_topk_ip_wide_i8", "clipmi_topk_ip_wide_workspace_bytes", 1024)
