"""The item-embedding modules of the research path (research/modeling/sequential/embedding_modules.py): plain
``torch.nn.Embedding`` lookups with row 0 as the padding row -- same class, constructor-argument, parameter and buffer
names as the reference, so its state_dicts load with ``strict=True``."""

import abc

import torch

from generative_recommenders_amd.research.modeling.initialization import truncated_normal


class EmbeddingModule(torch.nn.Module):
    @abc.abstractmethod
    def debug_str(self) -> str:
        pass

    @abc.abstractmethod
    def get_item_embeddings(self, item_ids: torch.Tensor) -> torch.Tensor:
        pass

    @property
    @abc.abstractmethod
    def item_embedding_dim(self) -> int:
        pass


def _init_item_tables(module: torch.nn.Module) -> None:
    for name, p in module.named_parameters():
        if "_item_emb" in name:
            truncated_normal(p, mean=0.0, std=0.02)


class LocalEmbeddingModule(EmbeddingModule):
    """ids 1 .. num_items, 0 is padding"""

    def __init__(self, num_items: int, item_embedding_dim: int) -> None:
        super().__init__()
        self._item_embedding_dim: int = item_embedding_dim
        self._item_emb = torch.nn.Embedding(num_items + 1, item_embedding_dim, padding_idx=0)
        self.reset_params()

    def debug_str(self) -> str:
        return f"local_emb_d{self._item_embedding_dim}"

    def reset_params(self) -> None:
        _init_item_tables(self)

    def get_item_embeddings(self, item_ids: torch.Tensor) -> torch.Tensor:
        return self._item_emb(item_ids)

    @property
    def item_embedding_dim(self) -> int:
        return self._item_embedding_dim


class CategoricalEmbeddingModule(EmbeddingModule):
    """one row per category: item id i (1-based) reads row ``item_id_to_category_id[i - 1] + 1``; id 0 maps like id 1"""

    def __init__(self, num_items: int, item_embedding_dim: int, item_id_to_category_id: torch.Tensor) -> None:
        super().__init__()
        self._item_embedding_dim: int = item_embedding_dim
        self._item_emb: torch.nn.Embedding = torch.nn.Embedding(num_items + 1, item_embedding_dim, padding_idx=0)
        self.register_buffer("_item_id_to_category_id", item_id_to_category_id)
        self.reset_params()

    def debug_str(self) -> str:
        return f"cat_emb_d{self._item_embedding_dim}"

    def reset_params(self) -> None:
        _init_item_tables(self)

    def get_item_embeddings(self, item_ids: torch.Tensor) -> torch.Tensor:
        categories = self._item_id_to_category_id[(item_ids - 1).clamp(min=0)] + 1
        return self._item_emb(categories)

    @property
    def item_embedding_dim(self) -> int:
        return self._item_embedding_dim
