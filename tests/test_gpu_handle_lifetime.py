"""The one lifetime of the four handle classes (_lib.Handle) on real handles, each at the smallest input its constructor
takes: open, close, close again, and a method after close is a ValueError raised before the library is entered."""
import numpy as np
import pytest

from scrna_seq_qannealing_clustering_amd import annotate, preprocess, umap
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu

OPEN = {
    "Problem": (lambda: Problem.dense(np.zeros((4, 4), dtype=np.float32)), lambda p: p.sync()),
    "ExpressionMatrix": (lambda: preprocess.ExpressionMatrix(np.ones((8, 4), dtype=np.float32)), lambda m: m.normalize()),
    "FuzzyGraph": (lambda: umap.FuzzyGraph(np.array([[0.0], [1.0]], dtype=np.float32), 2), lambda g: g.fetch_knn()),
    "Annotator": (lambda: annotate.Annotator(np.ones((1, 1), dtype=np.float32), [0], 1), lambda a: a.score(np.ones((1, 1)))),
}


@pytest.mark.parametrize("kind", list(OPEN))
def test_open_close_close_again_then_refuse(kind):
    make, use = OPEN[kind]
    h = make()
    assert h._handle().value
    if kind == "ExpressionMatrix":
        assert h.device_bytes() > 0
    h.close()
    h.close()
    assert h._h is None
    with pytest.raises(ValueError, match="the %s is closed" % kind):
        use(h)
    with make() as again:                                      # a second handle of the kind opens after the first is gone
        assert again._handle().value
    with pytest.raises(ValueError, match="the %s is closed" % kind):
        again._handle()
