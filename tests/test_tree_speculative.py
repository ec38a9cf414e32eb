"""Host logic of tree speculative decoding (speculative.accept_tree, NgramTreeDrafter) on hand-made cases."""
import pytest

from distributed_inference_demo_amd.speculative import NgramTreeDrafter, accept_tree

#            0   1   2   3   4   5   6
TOKENS = [9, 20, 21, 30, 31, 40, 41]
PARENTS = [-1, 0, 0, 2, 2, 4, 0]


@pytest.mark.parametrize("top,visited,emitted", [
    ([21, 0, 31, 0, 40, 77, 0], [0, 2, 4, 5], [21, 31, 40, 77]),   # non-first children, down to a leaf
    ([20, 55, 0, 0, 0, 0, 0], [0, 1], [20, 55]),                   # a leaf at depth 1
    ([50, 0, 0, 0, 0, 0, 0], [0], [50]),                           # nothing accepted: the target's own token
    ([21, 0, 30, 8, 0, 0, 0], [0, 2, 3], [21, 30, 8]),             # the first child of an inner node
    ([41, 0, 0, 0, 0, 0, 6], [0, 6], [41, 6]),                     # the root's last child
])
def test_accept_tree(top, visited, emitted):
    assert accept_tree(TOKENS, PARENTS, top) == (visited, emitted)
    with pytest.raises(ValueError):
        accept_tree(TOKENS, PARENTS, top[:-1])


def test_ngram_tree_merges_the_continuations_most_recent_first():
    #     a  b  c  d     a  b  c  e  f     a  b  x     a  b
    h = [1, 2, 3, 4, 0, 1, 2, 3, 5, 6, 0, 1, 2, 7, 0, 1, 2]
    toks, par = NgramTreeDrafter(8, n_max=2).propose(h)
    # suffix (1, 2): occurrences at 11 (-> 7 0 1 2), 5 (-> 3 5 6 0 ...), 0 (-> 3 4 ...), merged under the last token
    assert toks == [2, 7, 0, 1, 2, 3, 5, 6] and par == [-1, 0, 1, 2, 3, 0, 5, 6]
    toks, par = NgramTreeDrafter(16, n_max=2).propose(h, 4)
    assert toks == [2, 7, 0, 1] and par == [-1, 0, 1, 2]
    # shared first token: the two (1, 2, 3, ...) continuations share the node of 3 and split below it
    toks, par = NgramTreeDrafter(7, n_max=3).propose(h[:10] + [1, 2])
    assert toks == [2, 3, 5, 6, 1, 2, 4] and par == [-1, 0, 1, 2, 3, 4, 1]
    assert NgramTreeDrafter(4).propose([1, 2, 3, 4]) is None and NgramTreeDrafter(4).propose([5]) is None
    with pytest.raises(ValueError):
        NgramTreeDrafter(17)
