"""CPU: near-duplicate detection without a GPU -- the tokenizer against the reference's own, the band search, the restatement's
answers on the corpus families, the C ABI's argument checks, and the CLI's grouping with the index replaced by the restatement.

tests/dedup_ref.py restates the specification of DESIGN.md "Near-duplicate detection".  The reference delegates that arithmetic
to `datasketch`, which is not a dependency of this project and could not be run against it: the signatures are UNPINNED against datasketch itself.
SHA-1 is pinned to `hashlib`, the tokenizer to the reference's own function (tests/golden/make_golden_dedup.py)."""
import collections
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

from tests import dedup_ref as R
from tests.dedup_cases import token_set_corpus


def _golden(golden_dir):
    with gzip.open(os.path.join(golden_dir, "dedup_tokens.json.gz")) as f:
        return json.loads(f.read().decode("utf-8"))["cases"]


def test_tokenizer_equals_the_references(golden_dir, tmp_path):
    from buglab.data.deduplication import python_dedup_tokenize_file, python_dedup_tokenize_text

    cases = _golden(golden_dir)
    assert len(cases) >= 10
    for i, case in enumerate(cases):
        assert python_dedup_tokenize_text(case["text"]) == case["tokens"], i
        assert python_dedup_tokenize_text(case["text"], all_tokens=True) == case["all_tokens"], i
        path = tmp_path / f"case_{i}.py"
        path.write_text(case["text"], encoding="utf-8")
        assert python_dedup_tokenize_file(str(path)) == {"filename": str(path), "tokens": case["tokens"]}
        assert python_dedup_tokenize_file(str(path), all_tokens=True)["tokens"] == case["all_tokens"]
    broken = cases[-1]  # stops tokenizing half way: what was read is kept, the rest is not
    assert "third_value" in broken["tokens"] and "fourth_value" not in broken["tokens"] and "fourth_value" in broken["text"]
    assert all("def" not in c["tokens"] and "def" not in c["all_tokens"] for c in cases)  # keywords are left out in both modes
    assert any("(" in c["all_tokens"] and "(" not in c["tokens"] for c in cases)
    assert python_dedup_tokenize_file(str(tmp_path / "missing.py"))["tokens"] == []


def test_band_search():
    from buglab.data.deduplication import optimal_bands

    assert optimal_bands(0.85, 256) == (13, 19) == R.optimal_bands(0.85, 256)
    for setting, literal in (((0.5, 128), (25, 5)), ((0.9, 64), (3, 21))):
        assert optimal_bands(*setting) == literal == R.optimal_bands(*setting) and literal[0] * literal[1] <= setting[1]


def test_permutations_and_token_hash_follow_the_specification():
    from buglab.data.deduplication.index import permutations

    a, b = R.permutations(256)
    # rows in order, a then b: the second row's a follows the first row's b in the generator's stream
    assert (int(a[0]), int(b[0]), int(a[1])) == (775169054918279404, 1758426461858698312, 2109959069025162)
    a2, b2 = permutations(256)
    assert a2.dtype == np.uint64 and np.array_equal(a, a2) and np.array_equal(b, b2)
    assert np.array_equal(R.permutations(128)[0], a[:128])
    assert R.token_hash("") == 0xEEA339DA  # SHA-1("") = da39a3ee...
    assert R.token_hash("abc") == 0x363E99A9  # SHA-1("abc") = a9993e36...
    # the product wraps at 64 bits before the Mersenne reduction
    sig = R.signature(["abc"], (a, b))
    k = 0
    assert int(sig[k]) == (((int(a[k]) * 0x363E99A9 + int(b[k])) % (1 << 64)) % ((1 << 61) - 1)) & 0xFFFFFFFF
    assert int(sig[k]) != ((int(a[k]) * 0x363E99A9 + int(b[k])) % ((1 << 61) - 1)) & 0xFFFFFFFF


def test_restatement_flags_the_corpus_families():
    """200-token sets: an exact copy and 5 of 200 replaced (Jaccard 0.95) are flagged, every one; 40 of 200 replaced (Jaccard 0.67)
    and unrelated documents never; too-short documents never and they are not inserted; a repeated filename is flagged unless
    its first bearer was too short.  (Between the two replaced counts the answer is probabilistic and is not asserted.)"""
    names, sets, families = token_set_corpus(320, seed=3)
    index = R.RefDuplicationIndex()
    flags = index.check_batch(names, sets)
    by_family = collections.defaultdict(list)
    for family, flag in zip(families, flags):
        by_family[family].append(bool(flag))
    assert len(by_family["near"]) >= 20 and len(by_family["far"]) >= 20
    assert all(by_family["copy"]) and all(by_family["near"])
    assert not any(by_family["far"]) and not any(by_family["base"]) and not any(by_family["short"])
    inserted = set()
    for name, tokens, family, flag in zip(names, sets, families, flags):
        if family == "repeat":
            assert flag == (name in inserted)
        if len(tokens) >= 10:
            inserted.add(name)
    assert len(index) == len(inserted)
    # one at a time == the batch, and collisions name the source of a copy
    again = R.RefDuplicationIndex()
    assert [again.check_if_duplicate_and_add(n, s) for n, s in zip(names, sets)] == list(flags)
    copies = [n for n, f in zip(names, families) if f == "copy"]
    assert all(len(v) >= 1 for v in index.collisions(copies).values())


def test_restatement_on_tokenized_functions():
    """make_dedup_corpus through the tokenizer: copies under another path and 2 of 150 identifiers renamed are flagged, half of
    them renamed and unrelated functions are not, short ones are not."""
    from buglab.data.deduplication import python_dedup_tokenize_text
    from buglab.data.synthetic import make_dedup_corpus

    datapoints, functions = make_dedup_corpus(64, seed=1)
    assert len(datapoints) == 3 * 64
    first_text = {}
    for p in datapoints:
        first_text.setdefault((p["package_name"], p["graph"]["path"], tuple(p["graph"]["code_range"][0])), p["graph"]["text"])
    assert len(first_text) == 64
    index = R.RefDuplicationIndex()
    for fn in functions:
        tokens = set(python_dedup_tokenize_text(first_text[(fn["package_name"], fn["path"], fn["start"])]))
        flag = index.check_if_duplicate_and_add(fn["path"], tokens)
        expected = fn["family"] == "copy" or (fn["family"] == "rename" and fn["k"] == 2)
        assert flag == expected, fn
        assert (len(tokens) < 10) == (fn["family"] == "short")


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bl_dedup_sha1_u32(p, 8, None, 2, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_dedup_sha1_u32(None, 8, p, 2, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_dedup_minhash(p, 4, p, 1, None, p, 256, p, None) == -1 and b"null" in lib.bl_last_error()
    for num_perm in (0, 257, 512):  # not covered by the kernel: one permutation per lane of one workgroup
        assert lib.bl_dedup_minhash(p, 4, p, 1, p, p, num_perm, p, None) == -1 and b"num_perm" in lib.bl_last_error()
        assert lib.bl_dedup_lsh_insert_query(p, num_perm, 1, 1, p, 1024, 0, 0, 4, p, p, None) == -1 and b"num_perm" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(p, 256, 13, 20, p, 1024, 0, 0, 4, p, p, None) == -1  # b * r > num_perm
    assert b"does not fit num_perm" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(p, 256, 13, 19, p, 1000, 0, 0, 4, p, p, None) == -1 and b"power of two" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(p, 256, 13, 19, p, 1024, 0, 0, 513, p, p, None) == -1 and b"load bound" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(p, 256, 13, 19, p, 1024, 5, 0, 4, p, p, None) == -1 and b"insert_from" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(None, 256, 13, 19, p, 1024, 0, 0, 4, p, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_dedup_lsh_insert_query(p, 256, 13, 19, p, 1024, 0, 0, 4, None, p, None) == -1 and b"null flags" in lib.bl_last_error()
    with pytest.raises(hip_ops.HipOpsUnavailable):  # the wrappers take device tensors only: no CPU fallback
        import torch

        hip_ops.dedup_sha1_u32(torch.zeros(4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))


# ---- the CLI with the index replaced by the restatement ---------------------------------------------------------------------
def _write_shards(datapoints, directory, per_shard=40):
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    os.makedirs(directory, exist_ok=True)
    for i in range(0, len(datapoints), per_shard):
        save_msgpack_l_gz(datapoints[i:i + per_shard], os.path.join(directory, f"shard-{i // per_shard:03d}.msgpack.l.gz"))


def _ref_index(args):
    return R.RefDuplicationIndex(duplication_jaccard_threshold=args.threshold, num_perm=args.num_perm, min_num_tokens=args.min_num_tokens)


def test_cli_arguments(tmp_path):
    from buglab.data.deduplication.__main__ import default_workers, parse_args

    data, other = tmp_path / "data", tmp_path / "other"
    data.mkdir(), other.mkdir()
    args = parse_args([str(data), str(tmp_path / "out")])
    assert (args.threshold, args.num_perm, args.min_num_tokens, args.all_tokens, args.batch_size, args.against, args.workers) == \
        (0.85, 256, 10, False, 4096, [], None)
    args = parse_args([str(data), str(tmp_path / "out"), "--against", str(other), "--against", str(data), "--threshold", "0.7", "--num-perm",
                       "128", "--min-num-tokens", "5", "--all-tokens", "--report-json", "r.json", "--batch-size", "7", "--workers", "2"])
    assert (args.threshold, args.num_perm, args.min_num_tokens, args.all_tokens, args.batch_size, args.workers) == (0.7, 128, 5, True, 7, 2)
    assert args.against == [str(other), str(data)] and args.report_json == "r.json"
    for bad in (["--threshold", "1.5"], ["--batch-size", "0"], ["--workers", "17"], ["--against", str(tmp_path / "nowhere")], ["--num-perm", "1"], ["--num-perm", "257"]):
        with pytest.raises(SystemExit):
            parse_args([str(data), str(tmp_path / "out")] + bad)
    with pytest.raises(SystemExit):
        parse_args([str(data), str(data)])
    with pytest.raises(SystemExit):
        parse_args([str(tmp_path / "nowhere"), str(tmp_path / "out")])
    assert 1 <= default_workers() <= min(16, len(os.sched_getaffinity(0)))


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_groups_datapoints_by_function(tmp_path, workers):
    """A document is a function: its rewrites never count against it, all of a key's datapoints are kept or dropped together
    (also where they are not adjacent), and the answers are the restatement's on the first datapoint's text."""
    from buglab.data.deduplication import python_dedup_tokenize_text
    from buglab.data.deduplication.__main__ import document_key, main
    from buglab.data.synthetic import make_dedup_corpus
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    datapoints, functions = make_dedup_corpus(72, seed=2)
    _write_shards(datapoints, tmp_path / "data")
    report = main([str(tmp_path / "data"), str(tmp_path / "out"), "--report-json", str(tmp_path / "report.json"), "--batch-size", "10",
                   "--workers", str(workers)], make_index=_ref_index)

    expected = R.RefDuplicationIndex()
    texts = collections.OrderedDict()
    for p in load_all_msgpack_l_gz(str(tmp_path / "data")):
        texts.setdefault(document_key(p), p["graph"]["text"])
    assert len(texts) == 72
    flags = {k: expected.check_if_duplicate_and_add(k, set(python_dedup_tokenize_text(t))) for k, t in texts.items()}
    dropped = {k for k, f in flags.items() if f}
    assert dropped and len(dropped) == sum(f["family"] == "copy" or (f["family"] == "rename" and f["k"] == 2) for f in functions)

    kept = collections.Counter(document_key(p) for p in load_all_msgpack_l_gz(str(tmp_path / "out")))
    assert set(kept) == set(texts) - dropped
    assert all(n == 3 for n in kept.values())  # every rewrite of a kept function is kept
    assert report == json.load(open(tmp_path / "report.json"))
    assert report["documents"] == 72 == report["kept"] + report["dropped"] and report["dropped"] == len(dropped)
    assert report["too_short"] == sum(f["family"] == "short" for f in functions) and report["duplicate_keys"] == 0
    assert report["datapoints_read"] == 3 * 72 and report["datapoints_kept"] == 3 * len(kept)
    assert {d["key"] for d in report["dropped_documents"]} == dropped
    assert all(d["collided_with"] and set(d["collided_with"]) <= set(texts) - {d["key"]} for d in report["dropped_documents"])
    assert report["workers"] == workers and set(report["seconds"]) == {"read", "tokenize", "index", "write"}


def test_cli_against_drops_functions_close_to_the_other_data(tmp_path):
    from buglab.data.deduplication.__main__ import document_key, main
    from buglab.data.synthetic import make_dedup_corpus
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    datapoints, functions = make_dedup_corpus(48, seed=4, scatter_keys=False)
    per_function = [datapoints[3 * i:3 * i + 3] for i in range(48)]
    # the "test set": every third function; the very same functions are also left in the data (duplicate keys)
    test_set = [p for i in range(0, 48, 3) for p in per_function[i]]
    _write_shards(datapoints, tmp_path / "data")
    _write_shards(test_set, tmp_path / "test")
    plain = main([str(tmp_path / "data"), str(tmp_path / "out_plain"), "--workers", "1"], make_index=_ref_index)
    report = main([str(tmp_path / "data"), str(tmp_path / "out"), "--against", str(tmp_path / "test"), "--against", str(tmp_path / "test"),
                   "--workers", "1"], make_index=_ref_index)
    in_test = {document_key(p) for p in test_set}
    long_in_test = {document_key(p) for i in range(0, 48, 3) if functions[i]["family"] != "short" for p in per_function[i]}
    assert report["against_documents"] == len(in_test) == 16
    assert report["duplicate_keys"] == len(long_in_test) > 0
    kept = {document_key(p) for p in load_all_msgpack_l_gz(str(tmp_path / "out"))}
    assert not (kept & long_in_test)  # nothing of the test set stays in the training data
    assert kept <= {document_key(p) for p in load_all_msgpack_l_gz(str(tmp_path / "out_plain"))}
    assert report["dropped"] > plain["dropped"] and report["documents"] == plain["documents"] == 48
    by_key = {d["key"]: d["collided_with"] for d in report["dropped_documents"]}
    assert all(by_key[k] == [k] for k in long_in_test)
    assert not any(os.path.basename(f).startswith("shard-") for f in os.listdir(tmp_path / "out"))
