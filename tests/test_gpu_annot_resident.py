"""Annotation on the resident expression handle (mi_annot_score_matrix, mi_annot_score_clusters, mi_annot_fetch_chunk;
csrc/annot_kernels.hip): the gathered chunk and the cluster means on their raw output, bit for bit; the chain after them
against ``Annotator.score`` on the densified columns, field for field; ``single_r`` on a handle against ``single_r`` on the
host matrix; refusals by code, with the state they leave.  Expected values come from host slices of the handle's own
fetched matrix, from the existing host-array path and from tests/annot_resident_reference.py, never from the new code."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import annot_resident_reference as rr
import sct_cases
from scrna_seq_qannealing_clustering_amd import _lib, annotate, preprocess

pytestmark = pytest.mark.gpu

N = rr.N
EINVAL, EUNSUPPORTED, ESTATE = -1, -5, -6
CHUNKS = [(0, N), (0, 1), (N - 1, N), (16, 33)]
WHICH = ("counts", "normalized")
SCORE_FIELDS = ("sab", "sa2", "sb2", "scores", "first_labels")
TUNE_FIELDS = ("labels", "tuned_best", "tuned_next", "iterations")


class Resident:
    """one matrix of tests/annot_resident_reference.py open as a dense and as a CSR handle, both normalised, with the dense
    host copy of each of their matrices (``host[kind][which]``: what the handle itself returns)"""

    def __init__(self, name):
        X = rr.matrix(name)
        self.g = X.shape[1]
        self.names = ["g%04d" % j for j in range(self.g)]
        self.handles = {"dense": preprocess.ExpressionMatrix(X).normalize(),
                        "csr": preprocess.ExpressionMatrix(rr.csr_with_stored_zeros(X, rr.marker_cols(self.g, 130))).normalize()}
        self.host = {}
        for kind, h in self.handles.items():
            counts, norm = h.fetch_counts(), h.fetch_normalized()
            self.host[kind] = {"counts": counts.toarray() if h.sparse else counts,
                               "normalized": norm.toarray() if h.sparse else norm}
            for v in self.host[kind].values():
                v.setflags(write=False)
        assert self.handles["csr"].sparse and not self.handles["dense"].sparse
        for w in WHICH:                                           # (the package's contract since the sparse handle exists)
            assert np.array_equal(self.host["dense"][w], self.host["csr"][w])

    def close(self):
        for h in self.handles.values():
            h.close()


@pytest.fixture(scope="module")
def resident():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Resident(name)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def dummy_annotator(m, seed=0):
    """an annotator over m genes with an arbitrary three-sample, two-label reference (the gather does not read it)"""
    rng = np.random.default_rng(seed + m)
    return annotate.Annotator(rng.random((3, m)).astype(np.float32), np.array([0, 1, 1], dtype=np.int32), 2)


def code_of(fn, *args, **kw):
    with pytest.raises(_lib.MiSaError) as ei:
        fn(*args, **kw)
    return ei.value.code


def assert_same(a, b, keys):
    for key in keys:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, key
        if x.dtype == object:
            assert all(p == q for p, q in zip(x, y)), key
        else:
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), key          # bit for bit


# ---- 1. the gather, raw -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["base", "wide"])
@pytest.mark.parametrize("m", rr.M_LIST)
def test_gathered_chunk_is_the_host_slice(resident, name, m):
    r = resident(name)
    cols = rr.marker_cols(r.g, m)
    with dummy_annotator(m) as ann:
        for which in WHICH:
            for i0, i1 in CHUNKS:
                got = {}
                for kind, h in r.handles.items():
                    ann.score_matrix(h, cols, i0, i1, which)
                    got[kind] = ann.fetch_chunk()
                    want = r.host[kind][which][i0:i1][:, cols]
                    assert got[kind].shape == want.shape and got[kind].dtype == np.float32
                    assert np.array_equal(got[kind].view(np.uint32), want.view(np.uint32)), (kind, which, i0, i1)
                assert np.array_equal(got["dense"].view(np.uint32), got["csr"].view(np.uint32))
    if name == "wide":
        assert (r.host["csr"]["counts"][rr.LONG_ROW] != 0).sum() == 700 > 256


# ---- 2. the chain on the gathered chunk -------------------------------------------------------------------------------------

def planted_setup(r):
    """-> (cols, annotator arguments) of the planted L = 3 reference on the "base" matrix's genes"""
    c = rr.planted()
    assert c.gene_names == r.names
    return annotate._marker_setup(r.names, c.ref)


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_chain_equals_score_on_the_densified_slice(resident, kind):
    r = resident("base")
    cols, ref_args = planted_setup(r)
    iterated = 0
    with annotate.Annotator(*ref_args) as ann, annotate.Annotator(*ref_args) as other:
        for which in WHICH:
            for i0, i1 in CHUNKS:
                got = ann.score_matrix(r.handles[kind], cols, i0, i1, which, integers=True)
                assert set(got["kernel_ms"]) == {"gather", "rank", "cross", "scores"}
                got.update(ann.fine_tune())
                want = other.score(np.ascontiguousarray(r.host[kind][which][i0:i1][:, cols]), integers=True)
                want.update(other.fine_tune())
                assert_same(got, want, SCORE_FIELDS + TUNE_FIELDS)
                iterated += int((got["iterations"] > 0).sum())
    assert iterated > 0                                          # fine-tuning had work to do


# ---- 3. single_r end to end -------------------------------------------------------------------------------------------------

RESULT_ARRAYS = ("labels", "first_labels", "pruned_labels", "label_ids", "scores", "tuned_best", "tuned_next", "iterations",
                 "delta")


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_single_r_on_a_handle_equals_single_r_on_the_host_matrix(resident, kind):
    r = resident("base")
    c = rr.planted()
    h = r.handles[kind]
    want = annotate.single_r(r.host[kind]["normalized"], r.names, c.ref)
    before = h.device_bytes()
    for chunk in (17, 64, annotate.MAX_CHUNK):
        got = annotate.single_r(h, r.names, c.ref, chunk=chunk)
        assert_same(got, want, RESULT_ARRAYS)
        assert got["marker_genes"] == want["marker_genes"] and got["label_values"] == want["label_values"]
        assert "gather" in got["kernel_ms"] and "gather" not in want["kernel_ms"]
    assert h.device_bytes() == before
    again = h.annotate(r.names, c.ref, chunk=17)                 # the convenience method; two runs, identical bits
    assert_same(again, want, RESULT_ARRAYS)
    counts = annotate.single_r(h, r.names, c.ref, which="counts")
    assert_same(counts, annotate.single_r(r.host[kind]["counts"], r.names, c.ref), RESULT_ARRAYS)


def test_single_r_on_the_corrected_handle_of_sctransform():
    X, groups, marker = sct_cases.planted_counts()
    names = ["g%04d" % j for j in range(X.shape[1])]
    rng = np.random.default_rng(8)
    profiles = np.stack([np.log1p(X[groups == c].mean(axis=0)) for c in range(3)])
    ref = annotate.Reference(np.repeat(profiles, 3, axis=0) + rng.normal(0.0, 0.05, (9, X.shape[1])), names,
                             np.repeat(["a", "b", "c"], 3), de_n=40)
    res = preprocess.sctransform(sp.csr_matrix(X), variable_features_n=200, npcs=10, return_corrected=True)
    with res["corrected"] as h:
        assert h.sparse and h.normalized
        want = annotate.single_r(h.fetch_normalized().toarray(), names, ref)
        for chunk in (64, annotate.MAX_CHUNK):
            assert_same(annotate.single_r(h, names, ref, which="normalized", chunk=chunk), want, RESULT_ARRAYS)


# ---- 4. the cluster means, raw ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["base", "wide"])
@pytest.mark.parametrize("K", rr.K_LIST)
def test_cluster_means_are_the_sequential_fp64_means(resident, name, K):
    r = resident(name)
    lab = rr.interleaved_labels(K)
    for m in (65, 130) if name == "base" else (130,):
        cols = rr.marker_cols(r.g, m, seed=K)
        for which in WHICH:
            got = {}
            for kind, h in r.handles.items():
                means, sizes = annotate.cluster_means(h, cols, lab, which)
                want, want_sizes = rr.cluster_means_reference(r.host[kind][which], cols, lab)
                assert means.dtype == np.float32 and means.shape == (K, m)
                assert sizes.dtype == np.int32 and np.array_equal(sizes, want_sizes)
                assert np.array_equal(means.view(np.uint32), want.view(np.uint32)), (kind, which, m)
                got[kind] = means
            assert np.array_equal(got["dense"].view(np.uint32), got["csr"].view(np.uint32))
            if K == N:                                           # every cell its own cluster: the rows themselves
                assert np.array_equal(got["dense"][lab], r.host["dense"][which][:, cols])


# ---- 5. clusters mode -------------------------------------------------------------------------------------------------------

CLUSTER_FIELDS = ("labels", "scores", "iterations", "tuned_best", "tuned_next")


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_clusters_mode_equals_single_r_on_the_mean_rows(resident, kind):
    r = resident("base")
    c = rr.planted()
    lab = ["cl%d" % (i % 7) for i in range(N)]                   # any hashable values, interleaved
    lab[11] = "alone"
    ids, values = annotate.encode_labels(lab)
    got = annotate.single_r(r.handles[kind], r.names, c.ref, clusters=lab)
    cols = [r.names.index(gname) for gname in got["marker_genes"]]
    means, sizes = rr.cluster_means_reference(r.host[kind]["normalized"], cols, ids)
    want = annotate.single_r(means, got["marker_genes"], c.ref)
    assert want["marker_genes"] == got["marker_genes"]
    assert_same(got, want, CLUSTER_FIELDS + ("pruned_labels", "delta"))
    assert got["cluster_values"] == values and np.array_equal(got["cluster_sizes"], sizes) and sizes[values.index("alone")] == 1
    assert got["scores"].shape == (8, c.ref.L) and len(got["cell_labels"]) == N
    assert all(got["cell_labels"][i] == got["labels"][ids[i]] for i in range(N))
    assert "means" in got["kernel_ms"]


@pytest.mark.parametrize("form", ["array", "scipy", "handle"])
def test_clusters_mode_names_the_planted_cell_types(form):
    c = rr.planted()
    lab = ["type_%02d" % t for t in c.truth]
    if form == "handle":
        with preprocess.ExpressionMatrix(c.X) as h:
            got = annotate.single_r(h, c.gene_names, c.ref, clusters=lab, which="counts")
    else:
        got = annotate.single_r(sp.csr_matrix(c.X) if form == "scipy" else c.X, c.gene_names, c.ref, clusters=lab)
    assert len(got["cluster_values"]) == c.L
    assert list(got["labels"]) == got["cluster_values"]          # every cluster gets its planted label
    assert list(got["cell_labels"]) == lab
    ids, _ = annotate.encode_labels(lab)
    means, _ = rr.cluster_means_reference(c.X, [c.gene_names.index(gname) for gname in got["marker_genes"]], ids)
    assert_same(got, annotate.single_r(means, got["marker_genes"], c.ref), CLUSTER_FIELDS)


# ---- 6. refusals and state --------------------------------------------------------------------------------------------------

def test_refusals_name_their_code_and_leave_no_chunk(resident):
    r = resident("base")
    h = r.handles["dense"]
    cols, ref_args = planted_setup(r)
    cols = cols.astype(np.int32)
    m = len(cols)
    assert m > 40
    lab = rr.interleaved_labels(2)
    repeated, past = cols.copy(), cols.copy()
    repeated[40] = repeated[3]
    past[9] = r.g
    empty, high = lab.copy(), lab.copy()
    empty[empty == 1] = 2                                        # K = 3 with cluster 1 unused
    high[4] = 2                                                  # a label equal to K = 2
    with annotate.Annotator(*ref_args) as ann, preprocess.ExpressionMatrix(rr.matrix("base")) as raw:
        lib = _lib.load()

        def raw_which(which):                                    # (the Python layer maps names to 0 / 1: call the export)
            return _lib.call("mi_annot_score_matrix", ann._handle(), h._handle(), which, cols, 0, 4, None, None, None, None,
                             None, None)
        refusals = [
            ("a repeated column", EINVAL, lambda: ann.score_matrix(h, repeated, 0, 4)),
            ("a column equal to g", EINVAL, lambda: ann.score_matrix(h, past, 0, 4)),
            ("rows past n", EINVAL, lambda: ann.score_matrix(h, cols, N - 3, N + 1)),
            ("a negative first row", EINVAL, lambda: ann.score_matrix(h, cols, -1, 3)),
            ("no rows", EINVAL, lambda: ann.score_matrix(h, cols, 4, 4)),
            ("which = 2", EINVAL, lambda: raw_which(2)),
            ("normalised before normalize()", ESTATE, lambda: ann.score_matrix(raw, cols, 0, 4, "normalized")),
            ("means before normalize()", ESTATE, lambda: ann.score_clusters(raw, cols, lab, 2, "normalized")),
            ("an empty cluster", EINVAL, lambda: ann.score_clusters(h, cols, empty, 3)),
            ("a label equal to K", EINVAL, lambda: ann.score_clusters(h, cols, high, 2)),
            ("a repeated column in clusters mode", EINVAL, lambda: ann.score_clusters(h, repeated, lab, 2)),
            ("too many clusters", EUNSUPPORTED, lambda: ann.score_clusters(h, cols, lab, annotate.MAX_CHUNK + 1)),
        ]
        fresh, scratch = None, np.empty(8 * m, dtype=np.float32)
        for what, code, call in refusals:
            good = ann.score_matrix(h, cols, 0, 8, integers=True)    # a chunk is resident ...
            good.update(ann.fine_tune())
            if fresh is None:
                fresh = good
            assert_same(good, fresh, SCORE_FIELDS + TUNE_FIELDS)     # ... and a good call after a refusal is a good call
            assert code_of(call) == code, what
            assert code_of(ann.fine_tune) == ESTATE, what            # the refused call dropped it: the wrapper says so,
            assert code_of(ann.fetch_chunk) == ESTATE, what
            assert lib.mi_annot_fine_tune(ann._handle(), None, None, None, None, None) == ESTATE, what   # ... and the library
            assert lib.mi_annot_fetch_chunk(ann._handle(), scratch.ctypes.data_as(C.POINTER(C.c_float))) == ESTATE, what
        ann.score_matrix(raw, cols, 0, 4, "counts")                  # the un-normalised handle serves its counts
        assert np.array_equal(ann.fetch_chunk(), rr.matrix("base")[0:4][:, cols])


def test_handle_bytes_and_bits_are_stable(resident):
    r = resident("wide")
    c_cols = rr.marker_cols(r.g, 130)
    lab = rr.interleaved_labels(65)
    for kind, h in r.handles.items():
        before = h.device_bytes()
        with dummy_annotator(130) as ann:
            runs = []
            for _ in range(2):
                a = ann.score_matrix(h, c_cols, 0, N, integers=True)
                b = ann.score_clusters(h, c_cols, lab, 65, integers=True)
                b["chunk"] = ann.fetch_chunk()
                runs.append((a, b))
            assert_same(runs[0][0], runs[1][0], SCORE_FIELDS)
            assert_same(runs[0][1], runs[1][1], SCORE_FIELDS + ("sizes", "chunk"))
        assert h.device_bytes() == before, kind


# ---- 7. one annotator, host chunks and handle chunks in turn ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_alternating_host_and_handle_chunks_leak_nothing(resident, kind):
    r = resident("base")
    cols, ref_args = planted_setup(r)
    Y = r.host[kind]["normalized"]
    steps = [("host", 0, 64), ("handle", 60, 70), ("host", 3, 8), ("handle", 0, 70), ("host", 40, 41), ("handle", 69, 70)]
    with annotate.Annotator(*ref_args) as ann:
        for how, i0, i1 in steps:                                # larger, then smaller
            if how == "host":
                got = ann.score(np.ascontiguousarray(Y[i0:i1][:, cols]), integers=True)
            else:
                got = ann.score_matrix(r.handles[kind], cols, i0, i1, integers=True)
            got.update(ann.fine_tune())
            with annotate.Annotator(*ref_args) as fresh:
                want = fresh.score(np.ascontiguousarray(Y[i0:i1][:, cols]), integers=True)
                want.update(fresh.fine_tune())
            assert_same(got, want, SCORE_FIELDS + TUNE_FIELDS)
            assert np.array_equal(ann.fetch_chunk(), Y[i0:i1][:, cols])
