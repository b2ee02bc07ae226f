"""Near-duplicate detection (reference buglab/data/deduplication/): a MinHash-LSH index whose arithmetic runs on the device
(csrc/bl_dedup.hip), the reference's dedup tokenizer, and `python -m buglab.data.deduplication` to filter `*.msgpack.l.gz` shards.
The index is imported on first use, so that tokenizer worker processes never load torch."""

__all__ = ["DuplicationIndex", "optimal_bands", "python_dedup_tokenize_text", "python_dedup_tokenize_file"]


def __getattr__(name):
    if name in ("DuplicationIndex", "optimal_bands"):
        from buglab.data.deduplication import index

        return getattr(index, name)
    if name in ("python_dedup_tokenize_text", "python_dedup_tokenize_file"):
        from buglab.data.deduplication import tokenizers

        return getattr(tokenizers, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
