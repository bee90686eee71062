"""chunk_sets, the multipart grouping rule of Coordinator::handle_message_bytes
as a pure function: one table of the rule's cases, the expectation written out
a row."""
import pytest

from xaynet_amd.ops.box import chunk_sets

A, B = b"\x0a" * 32, b"\x0b" * 32


def ch(cid, last=0, pk=A, mid=7, n=150):
    return (pk, 2, 1, cid, mid, last, n)


CASES = {
    # name: (entries, sets, host_sets, pending)
    "in order": ([ch(0), ch(1), ch(2, 1)], [[0, 1, 2]], [], []),
    "reversed": ([ch(2, 1), ch(1), ch(0)], [[2, 1, 0]], [], []),
    "duplicate": ([ch(1), ch(0), ch(1), ch(2, 1)], [[1, 2, 3]], [], []),
    "two last ids": ([ch(0), ch(2, 1), ch(3, 1), ch(1)], [], [], [3]),
    "id beyond last, gap": ([ch(0), ch(3), ch(2, 1)], [], [], []),
    "chunk after completion": ([ch(0), ch(1, 1), ch(0)], [[0, 1]], [], [2]),
    "two participants, one id": ([ch(0), ch(0, pk=B), ch(1, 1, pk=B), ch(1, 1)],
                                 [[1, 2], [0, 3]], [], []),
    "no chunk": ([(A, 2, 0, 0, 0, 0, 300), ch(0)], [[0]], [], [1]),
    "short chunk 0": ([ch(1, 1), ch(0, n=135)], [], [[1, 0]], []),
}


@pytest.mark.parametrize("name", CASES)
def test_chunk_sets(name):
    entries, sets, host_sets, pending = CASES[name]
    assert chunk_sets(entries) == (sets, host_sets, pending)
