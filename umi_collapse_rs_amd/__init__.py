"""MI355X-native drop-in for the UMI-collapse hot path of tkob-vh/umi-collapse-rs.

Product code: csrc/ (gfx950 HIP kernels + the C ABI of include/umihip.h) and this
thin host-side mirror of the reference's Algorithm / DataStruct interface.  There
is no CPU fallback: without libumihip.so and a gfx950 device every compute call
raises UmiHipError."""
from ._lib import (LIB_PATH, UMI_ALGO_ADJACENCY, UMI_ALGO_CLUSTER, UMI_ALGO_DIRECTIONAL, UMI_CELLS_CR22, UMI_CELLS_MIN, UMI_CELLS_TOP,
                   UMI_GENE_ASSIGNED, UMI_GENE_NONE, UMI_GENE_SEVERAL, UMI_STRAND_FORWARD, UMI_STRAND_REVERSE, UMI_STRAND_UNSTRANDED,
                   UMI_INTRONS_OFF, UMI_INTRONS_EXON_FIRST, UMI_INTRONS_ALL, UMI_GENE_TIER_EXON, UMI_GENE_TIER_INTRON,
                   UMI_READ_CLASS_NONE, UMI_READ_CLASS_EXONIC, UMI_READ_CLASS_JUNCTION, UMI_READ_CLASS_SPANNING,
                   UMI_READ_CLASS_INTRONIC, UMI_READ_UNSTAGED, SATURATION_COLUMNS,
                   UMI_KERNEL_EDIT_PAIRS, UMI_MAX_UMI_LEN, Stats,
                   UmiHipError, load)
from .api import Adjacency, Cluster, Context, Directional, HipNaive, ReadFreq, default_context, to_bitset, to_bitset_seq

__all__ = ["LIB_PATH", "UMI_ALGO_ADJACENCY", "UMI_ALGO_CLUSTER", "UMI_ALGO_DIRECTIONAL", "UMI_CELLS_CR22", "UMI_CELLS_MIN",
           "UMI_CELLS_TOP", "UMI_GENE_ASSIGNED", "UMI_GENE_NONE", "UMI_GENE_SEVERAL", "UMI_STRAND_FORWARD", "UMI_STRAND_REVERSE",
           "UMI_STRAND_UNSTRANDED", "UMI_INTRONS_OFF", "UMI_INTRONS_EXON_FIRST", "UMI_INTRONS_ALL", "UMI_GENE_TIER_EXON",
           "UMI_GENE_TIER_INTRON", "UMI_READ_CLASS_NONE", "UMI_READ_CLASS_EXONIC", "UMI_READ_CLASS_JUNCTION",
           "UMI_READ_CLASS_SPANNING", "UMI_READ_CLASS_INTRONIC", "UMI_READ_UNSTAGED", "SATURATION_COLUMNS", "UMI_KERNEL_EDIT_PAIRS", "UMI_MAX_UMI_LEN", "Stats",
           "UmiHipError", "load", "Adjacency", "Cluster", "Context", "Directional", "HipNaive", "ReadFreq",
           "default_context", "to_bitset", "to_bitset_seq"]
