"""Drop-in for research/modeling/similarity_utils.py: the factories of the research path's similarity modules.  Same
arguments and debug strings as the reference's; plain functions (the reference's are gin-configurable)."""

from typing import List, Optional, Tuple

import torch

from generative_recommenders_amd.research.rails.similarities.dot_product_similarity_fn import DotProductSimilarity
from generative_recommenders_amd.research.rails.similarities.layers import SwiGLU
from generative_recommenders_amd.research.rails.similarities.mol.item_embeddings_fn import RecoMoLItemEmbeddingsFn
from generative_recommenders_amd.research.rails.similarities.mol.query_embeddings_fn import RecoMoLQueryEmbeddingsFn
from generative_recommenders_amd.research.rails.similarities.mol.similarity_fn import MoLSimilarity, SoftmaxDropoutCombiner


def init_mlp_xavier_weights_zero_bias(m) -> None:
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight)
        if getattr(m, "bias", None) is not None:
            m.bias.data.fill_(0.0)


def _sequential(*layers: torch.nn.Module) -> torch.nn.Sequential:
    return torch.nn.Sequential(*layers).apply(init_mlp_xavier_weights_zero_bias)


def create_mol_interaction_module(
    query_embedding_dim: int,
    item_embedding_dim: int,
    dot_product_dimension: int,
    query_dot_product_groups: int,
    item_dot_product_groups: int,
    temperature: float,
    query_dropout_rate: float,
    query_hidden_dim: int,
    item_dropout_rate: float,
    item_hidden_dim: int,
    gating_query_hidden_dim: int,
    gating_qi_hidden_dim: int,
    gating_item_hidden_dim: int,
    softmax_dropout_rate: float,
    bf16_training: bool,
    gating_query_fn: bool = True,
    gating_item_fn: bool = True,
    dot_product_l2_norm: bool = True,
    query_nonlinearity: str = "geglu",
    item_nonlinearity: str = "geglu",
    uid_dropout_rate: float = 0.5,
    uid_embedding_hash_sizes: Optional[List[int]] = None,
    uid_embedding_level_dropout: bool = False,
    gating_combination_type: str = "glu_silu",
    gating_item_dropout_rate: float = 0.0,
    gating_qi_dropout_rate: float = 0.0,
    eps: float = 1e-6,
) -> Tuple[MoLSimilarity, str]:
    """The MoL similarity of the reference's experiments and its debug string.  As there, the component projections are
    Dropout -> SwiGLU -> Linear whatever ``*_nonlinearity`` says (the strings only reach the debug string), and the uid
    arguments are accepted but not forwarded."""

    def component_proj(dropout_rate: float, hidden_dim: int):
        return lambda i, o: _sequential(torch.nn.Dropout(p=dropout_rate), SwiGLU(in_features=i, out_features=hidden_dim),
                                        torch.nn.Linear(in_features=hidden_dim, out_features=o))

    def gating_partial(hidden_dim: int, dropout_rate: Optional[float], bias: bool):
        def make(i: int, o: int) -> torch.nn.Sequential:
            head = [] if dropout_rate is None else [torch.nn.Dropout(p=dropout_rate)]
            if hidden_dim <= 0:
                return _sequential(*head, torch.nn.Linear(in_features=i, out_features=o))
            return _sequential(*head, torch.nn.Linear(in_features=i, out_features=hidden_dim), torch.nn.SiLU(),
                               torch.nn.Linear(in_features=hidden_dim, out_features=o, bias=bias))
        return make

    mol_module = MoLSimilarity(
        query_embedding_dim=query_embedding_dim,
        item_embedding_dim=item_embedding_dim,
        dot_product_dimension=dot_product_dimension,
        query_dot_product_groups=query_dot_product_groups,
        item_dot_product_groups=item_dot_product_groups,
        temperature=temperature,
        dot_product_l2_norm=dot_product_l2_norm,
        query_embeddings_fn=RecoMoLQueryEmbeddingsFn(
            query_embedding_dim=query_embedding_dim, query_dot_product_groups=query_dot_product_groups,
            dot_product_dimension=dot_product_dimension, dot_product_l2_norm=dot_product_l2_norm,
            proj_fn=component_proj(query_dropout_rate, query_hidden_dim), eps=eps),
        item_embeddings_fn=RecoMoLItemEmbeddingsFn(
            item_embedding_dim=item_embedding_dim, item_dot_product_groups=item_dot_product_groups,
            dot_product_dimension=dot_product_dimension, dot_product_l2_norm=dot_product_l2_norm,
            proj_fn=component_proj(item_dropout_rate, item_hidden_dim), eps=eps),
        gating_query_only_partial_fn=gating_partial(gating_query_hidden_dim, None, bias=False) if gating_query_fn else None,
        gating_item_only_partial_fn=(gating_partial(gating_item_hidden_dim, gating_item_dropout_rate, bias=False)
                                     if gating_item_fn else None),
        gating_qi_partial_fn=gating_partial(gating_qi_hidden_dim, gating_qi_dropout_rate, bias=True),
        gating_combination_type=gating_combination_type,
        gating_normalization_fn=lambda _: SoftmaxDropoutCombiner(dropout_rate=softmax_dropout_rate, eps=1e-6),
        eps=eps,
        autocast_bf16=bf16_training,
    )
    debug_str = (
        f"MoL-{query_dot_product_groups}x{item_dot_product_groups}x{dot_product_dimension}"
        f"-t{temperature}-d{softmax_dropout_rate}"
        f"{'-l2' if dot_product_l2_norm else ''}"
        f"-q{query_hidden_dim}d{query_dropout_rate}{query_nonlinearity}"
        f"-i{item_hidden_dim}d{item_dropout_rate}{item_nonlinearity}"
        + (f"-gq{gating_query_hidden_dim}" if gating_query_fn else "")
        + (f"-gi{gating_item_hidden_dim}d{gating_item_dropout_rate}" if gating_item_fn else "")
        + f"-gqi{gating_qi_hidden_dim}d{gating_qi_dropout_rate}-x-{gating_combination_type}"
    )
    return mol_module, debug_str


def get_similarity_function(module_type: str, query_embedding_dim: int, item_embedding_dim: int, bf16_training: bool = False,
                            activation_checkpoint: bool = False, **mol_kwargs) -> Tuple[torch.nn.Module, str]:
    """``DotProduct`` or ``MoL``.  The reference leaves MoL's remaining arguments to gin; here they are ``mol_kwargs``."""
    if module_type == "DotProduct":
        return DotProductSimilarity(), "DotProduct"
    if module_type == "MoL":
        return create_mol_interaction_module(query_embedding_dim=query_embedding_dim, item_embedding_dim=item_embedding_dim,
                                             bf16_training=bf16_training, **mol_kwargs)
    raise ValueError(f"Unknown interaction_module_type {module_type}")
