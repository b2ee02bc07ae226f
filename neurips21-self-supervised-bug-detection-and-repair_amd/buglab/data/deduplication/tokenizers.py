"""The dedup tokenizer of reference buglab/data/deduplication/tokenizers.py:14-24: Python's own tokenizer, `NAME` and `STRING`
tokens (or tokens of every kind with `all_tokens`), keywords left out in both modes; a tokenizer error is logged and what was read
up to it is kept.  Standard library only: worker processes import this module alone."""
import io
import keyword
import logging
from tokenize import NAME, STRING, tokenize
from typing import List, TypedDict


class TokenizedFileData(TypedDict):
    filename: str
    tokens: List[str]


def _tokens(readline, what: str, all_tokens: bool) -> List[str]:
    tokens: List[str] = []
    try:
        for toknum, tokval, _, _, _ in tokenize(readline):
            if all_tokens or toknum in (NAME, STRING):
                if not keyword.iskeyword(tokval):
                    tokens.append(tokval)
    except Exception as e:
        logging.error("Error tokenizing %s because %s", what, e)
    return tokens


def python_dedup_tokenize_text(text: str, all_tokens: bool = False) -> List[str]:
    """The tokens of source text held in memory (a function's `graph["text"]`), by the rule of `python_dedup_tokenize_file`."""
    return _tokens(io.BytesIO(text.encode("utf-8")).readline, "<text>", all_tokens)


def python_dedup_tokenize_file(filepath: str, all_tokens: bool = False) -> TokenizedFileData:
    try:
        with open(filepath, "rb") as f:
            tokens = _tokens(f.readline, filepath, all_tokens)
    except OSError as e:
        logging.error("Error tokenizing %s because %s", filepath, e)
        tokens = []
    return dict(filename=filepath, tokens=tokens)


def tokenize_text_job(job):
    """(text, all_tokens) -> the distinct tokens, sorted: what a worker process sends back for one document."""
    text, all_tokens = job
    return sorted(set(python_dedup_tokenize_text(text, all_tokens)))
