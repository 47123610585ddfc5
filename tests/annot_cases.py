"""Planted annotation problems for the tests: L label profiles over g genes, each with a few dozen up-regulated genes; the
last `twins` labels are near-twins of the first ones (a handful of genes apart), so that fine-tuning has work to do; a few
log-normal reference samples per label; test cells as Poisson draws from a profile (or from a mixture of two, which keeps
both labels in play), log-normalised.  The reference's gene list overlaps the test's only partly and is in another order.
Every case and its CPU restatement (tests/annot_reference.py) is computed once per process and shared."""
import functools

import numpy as np

import annot_reference as ar
from scrna_seq_qannealing_clustering_amd import annotate


class Case:
    pass


def planted(L, per_label, g, n, seed, twins=0, cousins=0, up=30, twin_genes=6, cousin_genes=14, depth=1500.0, mixtures=0,
            extra_ref_genes=40, drop=25):
    rng = np.random.default_rng(seed)
    base = rng.gamma(2.0, 0.4, g)
    prof = np.tile(base, (L, 1))
    for l in range(L - twins - cousins):
        prof[l, rng.choice(g, up, replace=False)] += rng.uniform(1.0, 2.5, up)
    for t in range(cousins):                                       # label L - twins - 1 - t: a more distant relative of label t
        prof[L - twins - 1 - t] = prof[t]
        prof[L - twins - 1 - t, rng.choice(g, cousin_genes, replace=False)] += rng.uniform(0.8, 1.6, cousin_genes)
    for t in range(twins):                                         # label L - 1 - t is the twin of label t
        prof[L - 1 - t] = prof[t]
        prof[L - 1 - t, rng.choice(g, twin_genes, replace=False)] += rng.uniform(0.8, 1.6, twin_genes)
    c = Case()
    c.L, c.g, c.n = L, g, n
    c.ref_ids = np.repeat(np.arange(L), per_label).astype(np.int32)
    c.ref_labels = ["type_%02d" % l for l in c.ref_ids]
    R = prof[c.ref_ids] + rng.normal(0.0, 0.15, (L * per_label, g))
    c.truth = rng.integers(0, L, n).astype(np.int32)
    mix = prof[c.truth].copy()
    for i in range(min(mixtures, n)):                              # the first cells: half-and-half of their label and the next
        mix[i] = np.log1p(0.5 * (np.expm1(prof[c.truth[i]]) + np.expm1(prof[(c.truth[i] + 1) % L])))
    rate = np.expm1(mix)
    counts = rng.poisson(rate / rate.sum(axis=1, keepdims=True) * depth)
    c.X = np.log1p(counts / np.maximum(counts.sum(axis=1, keepdims=True), 1) * 1e4).astype(np.float32)
    c.gene_names = ["g%04d" % j for j in range(g)]
    # the reference: `drop` of the test's genes missing, `extra_ref_genes` of its own, columns shuffled
    keep = np.sort(rng.permutation(g)[: g - drop])
    order = rng.permutation(len(keep) + extra_ref_genes)
    cols = np.concatenate([R[:, keep], rng.normal(1.0, 0.5, (R.shape[0], extra_ref_genes))], axis=1)
    names = [c.gene_names[j] for j in keep] + ["r%04d" % j for j in range(extra_ref_genes)]
    c.R = np.ascontiguousarray(cols[:, order], dtype=np.float32)
    c.ref_gene_names = [names[j] for j in order]
    return c


SPECS = {
    "L2": dict(L=2, per_label=3, g=200, n=60, seed=11, up=20, mixtures=12, extra_ref_genes=10, drop=10),
    "L6": dict(L=6, per_label=4, g=600, n=300, seed=12, twins=2, cousins=1),
    "L64": dict(L=64, per_label=1, g=600, n=24, seed=13, up=12, depth=3000.0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the planted case with its restatement: c.ref (annotate.Reference), c.M / c.pairs on the common genes, c.XM / c.RM the
    two matrices on M, c.expect = annot_reference.annotate(...)"""
    c = planted(**SPECS[name])
    c.ref = annotate.Reference(c.R, c.ref_gene_names, c.ref_labels)
    c.test_idx, c.ref_idx = annotate.common_genes(c.gene_names, c.ref_gene_names)
    c.pairs, c.M = c.ref.markers_on(c.ref_idx)
    pos = {int(j): k for k, j in enumerate(c.M)}
    c.local_pairs = {ab: [pos[int(j)] for j in genes] for ab, genes in c.pairs.items()}
    c.XM = np.ascontiguousarray(c.X[:, c.test_idx[c.M]])
    c.RM = np.ascontiguousarray(c.R[:, c.ref_idx[c.M]])
    c.masks = annotate.pair_masks(c.pairs, c.M, c.L)
    c.expect = ar.annotate(c.XM, c.RM, c.ref.label_ids, c.L, c.local_pairs)
    for v in c.expect.values():
        v.setflags(write=False)
    return c
