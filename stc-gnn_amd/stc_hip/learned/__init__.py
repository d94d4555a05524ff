"""Learned spatial graphs on a sparsity pattern (``graph_mode='csr-learned'``): the generator's front end restricted to the stored entries
of the prior graph (``csr.py``; kernels ``csrc/stc_mgp_csr.hip``, ABI v41).  The operand that carries the learned values into the cells is
``stc_hip.graph.learned_csr_operand``; the rank-r fusion on value vectors is ``stc_hip.fusion.mixed_fusion_lr``."""
from .csr import mgp_csr_front, mgp_csr_supported, mgp_csr_score, mgp_csr_softmax  # noqa: F401

__all__ = ['mgp_csr_front', 'mgp_csr_supported', 'mgp_csr_score', 'mgp_csr_softmax']
