"""MI355X-native simulated-annealing sampler for the graph-partition clustering models of
michal7kw/scRNA_seq_QAnnealing_Clustering (drop-in for its D-Wave / neal sampler calls).

Public surface:
    MI355XSampler            dimod-style sampler: sample_qubo / sample / sample_ising / sample_dqm
    SampleSet                dimod.SampleSet look-alike
    build_bqm_qubo, build_bqm2_qubo, build_bqm3_cut_qubo, build_dqm_potts   model builders
    BinaryQuadraticModel, DiscreteQuadraticModel     stand-ins for the dimod classes
    clustering_bqm, clustering_bqm_2, clustering_bqm_3, clustering_dqm  reference-shaped drivers
    clustering_modularity    weighted modularity at a resolution (Seurat's FindClusters objective)
    clustering_modularity_sweep  the same at several resolutions in one GPU launch
    preprocess               counts -> log-normalised matrix -> variable genes -> scaled matrix -> PCA coordinates (module)
    umap, run_umap           Seurat's RunUMAP: kNN -> fuzzy graph -> deterministic layout (module and its driver)
    mapping                  held-out cells onto a clustered sample: cross kNN, label transfer, extend_labels (module);
                             umap.transform places them in a fitted embedding
    tsne, run_tsne           Seurat's RunTSNE: kNN -> perplexity calibration -> joint P -> exact-repulsion layout (module and
                             its driver)
    anchors                  Seurat's FindTransferAnchors / TransferData / MapQuery: anchor-based label and feature transfer
                             (module: find_transfer_anchors, transfer_data, map_query)
    annotate                 SingleR-style cell-type annotation against a labelled reference (module: Reference, single_r)
"""
from .bqm import BinaryQuadraticModel, DiscreteQuadraticModel
from .models import (PottsModel, QuboModel, add_size_window_penalty, build_bqm2_qubo,
                     build_bqm3_cut_qubo, build_bqm_qubo, build_dqm_potts, default_beta_range,
                     make_beta_schedule, qubo_dict_to_model)
from .sampleset import SampleSet

__all__ = [
    "MI355XSampler", "SampleSet", "QuboModel", "PottsModel", "BinaryQuadraticModel",
    "DiscreteQuadraticModel", "build_bqm_qubo", "build_bqm2_qubo", "build_bqm3_cut_qubo",
    "build_dqm_potts", "add_size_window_penalty", "default_beta_range", "make_beta_schedule",
    "qubo_dict_to_model", "preprocess", "umap", "run_umap", "mapping", "anchors", "annotate", "tsne", "run_tsne",
]


def __getattr__(name):
    # the sampler (and everything that needs the HIP library) is imported lazily so that the pure
    # model layer can be used for inspection without a GPU
    if name == "MI355XSampler":
        from .sampler import MI355XSampler
        return MI355XSampler
    if name in ("clustering_bqm", "clustering_bqm_2", "clustering_bqm_3", "clustering_dqm", "clustering_modularity",
                "clustering_modularity_sweep"):
        from . import clustering
        return getattr(clustering, name)
    if name in ("preprocess", "umap", "mapping", "anchors", "annotate", "tsne"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "run_umap":
        from .umap import run_umap
        return run_umap
    if name == "run_tsne":
        from .tsne import run_tsne
        return run_tsne
    raise AttributeError(name)
