#!/usr/bin/env python
"""Golden outputs of the REFERENCE's dedup tokenizer (buglab/data/deduplication/tokenizers.py::python_dedup_tokenize_file), run
unmodified from a checkout of the reference:

    python tests/golden/make_golden_dedup.py REFERENCE_CHECKOUT     # rewrites tests/golden/dedup_tokens.json.gz

The inputs are this repository's own synthetic texts (buglab.data.synthetic.make_dedup_corpus, plus one text whose indentation
stops the tokenizer half way), written to temporary files; the fixture holds each text and the token lists the reference returns
for it with `all_tokens` off and on.  The reference's tokenizers.py is loaded by file path: its package's __init__ imports zmq, and
buglab.utils imports chardet, neither of which the tokenizer calls; chardet gets a stand-in module with the one name that is imported."""
import gzip
import importlib.util
import json
import os
import sys
import tempfile
import types

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
PKG = os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd")

BROKEN = "def broken(first_value, second_value):\n        third_value = first_value\n    fourth_value = 'never seen'\n    return fourth_value\n"


def texts():
    sys.path.insert(0, PKG)
    from buglab.data.synthetic import make_dedup_corpus

    datapoints, _ = make_dedup_corpus(16, seed=5, num_identifiers=40, rewrites_per_function=1, scatter_keys=False)
    out = [p["graph"]["text"] for p in datapoints] + [BROKEN]
    sys.path.remove(PKG)
    for name in [m for m in sys.modules if m == "buglab" or m.startswith("buglab.")]:
        del sys.modules[name]
    return out


def reference_tokenizer(ref):
    chardet = types.ModuleType("chardet")
    chardet.UniversalDetector = type("UniversalDetector", (), {})  # the one name buglab.utils imports; never instantiated here
    sys.modules["chardet"] = chardet
    sys.path.insert(0, ref)
    spec = importlib.util.spec_from_file_location("reference_dedup_tokenizers", os.path.join(ref, "buglab", "data", "deduplication", "tokenizers.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.python_dedup_tokenize_file


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    cases = texts()
    tokenize_file = reference_tokenizer(sys.argv[1])
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, text in enumerate(cases):
            path = os.path.join(tmp, f"case_{i}.py")
            with open(path, "w", encoding="utf-8") as f:
                f.write(text)
            records.append({"text": text, "tokens": tokenize_file(path)["tokens"], "all_tokens": tokenize_file(path, all_tokens=True)["tokens"]})
    assert records[-1]["tokens"] and "fourth_value" not in records[-1]["tokens"], "the broken text must stop the tokenizer half way"
    with gzip.GzipFile(os.path.join(OUT, "dedup_tokens.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps({"python": sys.version.split()[0], "cases": records}).encode("utf-8"))
    print(f"{len(records)} cases, {sum(len(r['tokens']) for r in records)} tokens")


if __name__ == "__main__":
    main()
