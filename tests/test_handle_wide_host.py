"""The conditions the wide-handle GPU tests (tests/test_gpu_handle_wide.py) rest on, checked off the GPU on their inputs
(tests/handle_wide_cases.py), so that a changed generator fails here and the GPU tests cannot go blind:

- corrected counts: no value within 1e-9 of a half-integer at any shape (the nearest is printed); every wavefront's quarter
  of every chunk of ``chunk_compact`` holds a zero that becomes a count, a stored count that stays one and an unlisted gene;
  a row with entries in two chunks; more than 256 listed genes; cells of more than 256 stored entries and corrected rows of
  more than 256;
- deep cells: every cell stores more than 256 entries;
- Gram: the workspace constant of include/mi_prep.h and its Python mirror agree, ``batch < chunks`` at the tested shape, and
  the bound of ``prep_reference.gram_bound`` separates the mistakes a second pass can make (on the numpy restatement of Z:
  the device's differs from it by last bits of the normalised values only).

    test                                                     the loop whose turning it vouches for             turns from
    test_corrected_inputs_have_no_entry_next_to_a_half...    (the comparison by equality leaves nothing out)   --
    test_corrected_inputs_cover_every_quarter_and_chunk      chunk_compact's wavefronts 1 - 3; k_sct_csr_rows'  g > 1024; g > 4096;
                                                             second chunk; the gene table's second workgroup;  256 listed genes;
                                                             the row walks that step by 256                    256 entries in a row
    test_every_quarter_of_the_first_two_chunks_has_a_...     each wavefront's quarter at least a ballot wide    --
    test_row_shapes_carry_over_two_tiles                     k_prep_scan_counts over the rows                  n > 2048
    test_deep_cells_store_more_than_256_entries              csr_row_scatter's `e += 256`                      256 stored in a cell
    test_gram_workspace_constant_and_batch                   mi_prep_gram's second pass                        chunks > batch: n > 3584
    test_gram_bound_separates_the_mistakes_of_a_second_pass  (a wrong second pass is outside the bound)        at h = 4096"""
import os
import re

import numpy as np
import pytest

import handle_wide_cases as hw
import prep_reference as ref
import sct_correct_reference as cr
from scrna_seq_qannealing_clustering_amd import preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,g", hw.CORRECTED_SHAPES + hw.ROW_SHAPES)
def test_corrected_inputs_have_no_entry_next_to_a_half_integer(n, g):
    X, genes, par, lu, lu_ref, want, near = hw.corrected_case(n, g)
    v = cr.values(X[:, genes], *par, lu, lu_ref)
    frac = np.abs(np.abs(v - np.floor(v)) - 0.5)
    print("(%d, %d): nearest to a half-integer %.3g; stored per cell <= %d, corrected per row <= %d, listed %d"
          % (n, g, frac.min(), (X != 0).sum(axis=1).max(), (want != 0).sum(axis=1).max(), len(genes)))
    assert np.isfinite(v).all() and not near.any()
    assert len(set(genes.tolist())) == len(genes) and g - 1 in genes


@pytest.mark.parametrize("n,g", hw.CORRECTED_SHAPES)
def test_corrected_inputs_cover_every_quarter_and_chunk(n, g):
    X, genes, _, _, _, want, _ = hw.corrected_case(n, g)
    hw.assert_corrected_coverage(X, genes, want)
    assert len(hw.quarters(g)) == -(-g // hw.CORR_QUARTER)
    # a cell's stored entries and a corrected row's entries both pass 256: the row walks of normalize, the scatter, the
    # histogram and the transpose step more than once
    assert (X != 0).sum(axis=1).max() > 256 and (want != 0).sum(axis=1).max() > 256


def test_every_quarter_of_the_first_two_chunks_has_a_full_turn_in_some_shape():
    """the tail quarters of one and three columns (a wavefront's last, partial ballot) carry the weaker condition; the same
    wavefront's quarter is at least a ballot wide, under the full conditions, at another shape"""
    full = {(lo // hw.CORR_CHUNK, lo % hw.CORR_CHUNK // hw.CORR_QUARTER)
            for _, g in hw.CORRECTED_SHAPES for lo, hi in hw.quarters(g) if hi - lo >= 64}
    assert full >= {(c, q) for c in (0, 1) for q in range(4)}


def test_quarters():
    assert hw.quarters(1023) == [(0, 1023)]
    assert hw.quarters(1025) == [(0, 1024), (1024, 1025)]
    assert hw.quarters(4097)[-2:] == [(3072, 4096), (4096, 4097)]
    assert hw.quarters(8195)[-1] == (8192, 8195) and len(hw.quarters(8195)) == 9


@pytest.mark.parametrize("n,g", hw.ROW_SHAPES)
def test_row_shapes_carry_over_two_tiles(n, g):
    assert n > 2 * 1024                                           # k_prep_scan_counts: tiles of 1024 counts
    _, _, _, _, _, want, _ = hw.corrected_case(n, g)
    per_tile = [(want[t:t + 1024] != 0).sum() for t in range(0, n, 1024)]
    assert len(per_tile) == 3 and all(c > 0 for c in per_tile)   # every tile adds to the carry of the next


@pytest.mark.parametrize("kind", hw.DEEP_KINDS)
def test_deep_cells_store_more_than_256_entries(kind):
    X, A = hw.deep_case(kind)
    assert X.shape == A.shape == (hw.DEEP_N, hw.DEEP_G) and np.array_equal(A.toarray(), X)
    hw.assert_deep(kind, X, A)


def test_gram_workspace_constant_and_batch():
    hdr = open(os.path.join(ROOT, "include", "mi_prep.h")).read()
    m = re.search(r"#define\s+MI_PREP_GRAM_WORKSPACE\s+\((\d+)ll\s*<<\s*(\d+)\)", hdr)
    assert m and int(m.group(1)) << int(m.group(2)) == preprocess.GRAM_WORKSPACE
    assert int(re.search(r"#define\s+MI_PREP_GRAM_CHUNK\s+(\d+)", hdr).group(1)) == preprocess.GRAM_CHUNK
    src = open(os.path.join(ROOT, "scrna_seq_qannealing_clustering_amd", "csrc", "prep_kernels.hip")).read()
    assert "kGramWorkspace = (size_t)MI_PREP_GRAM_WORKSPACE" in src
    # what the issue of these tests worked out by hand
    assert hw.gram_batch(257) == 682 and hw.gram_batch(3000) == 13 and hw.gram_batch(4096) == 7
    assert (hw.GRAM_H, hw.GRAM_N) == (4096, 3585)
    batch, chunks = hw.gram_batch(hw.GRAM_H), hw.gram_chunks(hw.GRAM_N)
    assert batch < chunks == batch + 1                            # a second pass, of one chunk
    assert hw.gram_batch(2049) >= hw.gram_chunks(513)            # the odd-T shape stays one pass


def test_gram_bound_separates_the_mistakes_of_a_second_pass():
    X, genes = hw.gram_counts()
    Z = ref.scaled_from_normalized(ref.normalize(X), genes, 10.0)
    heavy = np.isin(genes, np.arange(hw.GRAM_H)[hw.GRAM_HEAVY])
    assert heavy.sum() == hw.GRAM_H // 4 and (Z[-1, heavy] == 10.0).all()      # the last cell is heavy: at the clip
    Z64 = Z.astype(np.float64)
    G64 = Z64.T @ Z64
    hw.assert_gram_bound_separates(Z, G64, ref.gram_bound(G64, preprocess.GRAM_CHUNK))
