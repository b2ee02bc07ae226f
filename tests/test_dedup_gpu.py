"""GPU: near-duplicate detection on the MI355X (csrc/bl_dedup.hip, buglab.data.deduplication) against the sequential
restatement tests/dedup_ref.py.  Everything is integer arithmetic: all comparisons are `array_equal`, no tolerance, and every
document of every corpus is compared.

The restatement follows the specification of DESIGN.md "Near-duplicate detection".  The reference delegates that arithmetic to
`datasketch`, which is not a dependency of this project and could not be run against it, so the signatures are UNPINNED against datasketch itself;
SHA-1 is pinned to `hashlib`, the tokenizer to the reference's own function (tests/test_dedup_host.py)."""
import collections
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

from tests import dedup_ref as R
from tests.dedup_cases import token_set_corpus

pytestmark = pytest.mark.gpu

CORPUS_DOCS = 3000


def _sha1_u32_device(tokens):
    from buglab.data.deduplication.index import pack_tokens
    from buglab.models import hip_ops

    token_bytes, tok_off, _ = pack_tokens([tokens])
    out = hip_ops.dedup_sha1_u32(torch.from_numpy(token_bytes.copy()).cuda(), torch.from_numpy(tok_off).cuda())
    return out.cpu().numpy().view(np.uint32)


def _sha1_u32_host(tokens):
    return np.array([struct.unpack("<I", hashlib.sha1(t.encode("utf-8")).digest()[:4])[0] for t in tokens], dtype=np.uint32)


def test_sha1_kernel_equals_hashlib():
    rng = np.random.default_rng(0)
    by_length = ["".join(chr(int(c)) for c in rng.integers(33, 127, size=n)) for n in range(0, 131)]  # every block-boundary case
    assert [len(t.encode()) for t in by_length] == list(range(131))
    assert np.array_equal(_sha1_u32_device(by_length), _sha1_u32_host(by_length))
    non_ascii = ["é", "中文标识符", "\U0001f600" * 14, "naïve_" * 10 + "ü", "Ω" * 28, "x" * 55 + "é", "\x00", "a\x00b", " "]
    assert np.array_equal(_sha1_u32_device(non_ascii), _sha1_u32_host(non_ascii))
    alphabet = np.array(list("abcXYZ_019 é中\U0001f600'\""))
    random_tokens = ["".join(rng.choice(alphabet, size=int(n))) for n in rng.integers(0, 200, size=10000)]
    got, want = _sha1_u32_device(random_tokens), _sha1_u32_host(random_tokens)
    assert got.shape == (10000,) and np.array_equal(got, want)
    assert _sha1_u32_device([]).shape == (0,)


@pytest.mark.parametrize("num_perm", [128, 256])
def test_signatures_equal_the_restatement(num_perm):
    from buglab.data.deduplication import DuplicationIndex

    rng = np.random.default_rng(num_perm)
    docs = [{f"t{int(x):x}_é" if i % 3 == 0 else f"name_{int(x)}" for i, x in enumerate(rng.integers(0, 1 << 50, size=n))}
            for n in (10, 200, 5000, 11, 1024, 1025, 2048)]
    assert [len(d) for d in docs[:3]] == [10, 200, 5000]
    index = DuplicationIndex(None, num_perm=num_perm)
    assert (index.bands, index.rows) == R.optimal_bands(0.85, num_perm)
    index.check_batch([f"doc{i}" for i in range(len(docs))], docs)
    perm = R.permutations(num_perm)
    want = np.stack([R.signature(d, perm) for d in docs])
    got = index.signatures()
    assert got.dtype == np.uint32 and got.shape == (len(docs), num_perm)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def corpus():
    names, sets, families = token_set_corpus(CORPUS_DOCS, seed=11)
    ref = R.RefDuplicationIndex()
    flags = ref.check_batch(names, sets)
    counts = collections.Counter(families)
    assert all(counts[f] >= 300 for f in ("base", "copy", "near", "far", "short", "repeat"))
    assert 0 < flags.sum() < len(flags)
    return names, sets, flags, ref


def _run(names, sets, batch, index=None):
    from buglab.data.deduplication import DuplicationIndex

    index = index if index is not None else DuplicationIndex(None)
    flags = [index.check_batch(names[lo:lo + batch], sets[lo:lo + batch]) for lo in range(0, len(names), batch)]
    return np.concatenate(flags), index


def test_flags_equal_the_restatement_for_every_batch_split(corpus):
    """One batch; batches of 1, 7 and 1000; the corpus twice on fresh indices; with repeated filenames and too-short documents mixed
    in (the corpus holds both); across several growths of the band index (it starts at 1024 slots per band for 512 documents)."""
    names, sets, want, ref = corpus
    one, index = _run(names, sets, len(names))
    assert one.dtype == bool and one.shape == want.shape
    assert np.array_equal(one, want)  # every document
    assert len(index) == len(ref) and index.filenames() == ref.filenames()
    assert index.rebuilds >= 1
    sigs = index.signatures()
    assert np.array_equal(sigs, ref.signatures())
    for batch in (1, 7, 1000):
        got, other = _run(names, sets, batch)
        assert np.array_equal(got, want), batch
        assert other.rebuilds >= 2 or batch == 1000
        assert np.array_equal(other.signatures(), sigs), batch  # identical from run to run and split to split
    again, index2 = _run(names, sets, len(names))
    assert np.array_equal(again, one) and np.array_equal(index2.signatures(), sigs)


def test_one_at_a_time_equals_check_batch(corpus):
    from buglab.data.deduplication import DuplicationIndex

    names, sets, want, ref = corpus
    index = DuplicationIndex(None)
    got = np.array([index.check_if_duplicate_and_add(f, s) for f, s in zip(names, sets)])  # the whole corpus, every document
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len(index) == len(ref) > 2048 and index.rebuilds == 2  # both growths happen on a one-document batch
    assert np.array_equal(index.signatures(), ref.signatures())


def test_growth_of_the_band_index(corpus):
    """The same answers whether the index grows inside a batch, between batches, or not at all after one big first batch."""
    names, sets, want, _ = corpus
    from buglab.data.deduplication import DuplicationIndex

    known, inserted = set(), []  # documents in the index after each document of the corpus
    for name, tokens in zip(names, sets):
        if len(tokens) >= 10:
            known.add(name)
        inserted.append(len(known))
    cut1, cut2 = inserted.index(500) + 1, inserted.index(530) + 1
    assert inserted[-1] > 2048  # the second table (4096 slots per band) is outgrown as well
    index = DuplicationIndex(None)
    got = [index.check_batch(names[:cut1], sets[:cut1])]
    assert len(index) == 500 and index.rebuilds == 0  # the first table has 1024 slots per band: up to 512 documents
    got.append(index.check_batch(names[cut1:cut2], sets[cut1:cut2]))
    assert len(index) == 530 and index.rebuilds == 1
    got.append(index.check_batch(names[cut2:], sets[cut2:]))
    assert len(index) == inserted[-1] and index.rebuilds == 2
    assert np.array_equal(np.concatenate(got), want)


def test_save_and_load_in_the_middle(corpus, tmp_path):
    from buglab.data.deduplication import DuplicationIndex

    names, sets, want, _ = corpus
    half = 1400
    path = tmp_path / "index.npz"
    index = DuplicationIndex(path)
    first = index.check_batch(names[:half], sets[:half])
    index.save()
    assert path.exists() and not (tmp_path / "index.npz.npz").exists()
    loaded = DuplicationIndex.load(path)
    assert len(loaded) == len(index) and loaded.filenames() == index.filenames()
    assert (loaded.bands, loaded.rows, loaded.min_num_tokens) == (index.bands, index.rows, index.min_num_tokens)
    assert np.array_equal(loaded.signatures(), index.signatures())
    rest = loaded.check_batch(names[half:], sets[half:])
    assert np.array_equal(np.concatenate([first, rest]), want)
    loaded.clear()
    assert len(loaded) == 0 and not loaded.check_if_duplicate_and_add(names[0], sets[0])
    odd = ["a", "a\x00", "a\x00\x00", "", "é中\U0001f600 "]  # names a fixed-width string array would merge or strip
    index.clear()
    index.check_batch(odd, sets[:len(odd)])
    index.save()
    assert DuplicationIndex.load(path).filenames() == odd


def test_collisions_name_the_earlier_documents(corpus):
    names, sets, want, ref = corpus
    got, index = _run(names[:900], sets[:900], 300)
    small = R.RefDuplicationIndex()
    small.check_batch(names[:900], sets[:900])
    asked = [n for n in dict.fromkeys(names[:900]) if n in set(small.filenames())][::7]
    assert index.collisions(asked) == small.collisions(asked)


def test_cli_end_to_end(tmp_path):
    """Written shards through `python -m buglab.data.deduplication`'s main on the device index, with and without --against:
    the kept keys are the restatement's, the rewrites of a kept function are all kept, the report's counts add up."""
    from buglab.data.deduplication.__main__ import document_key, main
    from buglab.data.synthetic import make_dedup_corpus
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    datapoints, functions = make_dedup_corpus(160, seed=6)
    test_points, _ = make_dedup_corpus(40, seed=6, scatter_keys=False)  # the same first functions: keys and texts repeat
    for name, points in (("data", datapoints), ("test", test_points)):
        os.makedirs(tmp_path / name)
        for i in range(0, len(points), 100):
            save_msgpack_l_gz(points[i:i + 100], tmp_path / name / f"shard-{i // 100:03d}.msgpack.l.gz")

    def ref_index(args):
        return R.RefDuplicationIndex(duplication_jaccard_threshold=args.threshold, num_perm=args.num_perm, min_num_tokens=args.min_num_tokens)

    for extra in ([], ["--against", str(tmp_path / "test")]):
        tag = "against" if extra else "plain"
        argv = [str(tmp_path / "data"), None, "--batch-size", "37", "--workers", "2"] + extra
        argv[1] = str(tmp_path / f"out_{tag}")
        report = main(argv)
        argv[1] = str(tmp_path / f"ref_{tag}")
        want = main(argv, make_index=ref_index)
        kept = collections.Counter(document_key(p) for p in load_all_msgpack_l_gz(argv[1].replace("ref_", "out_")))
        kept_ref = collections.Counter(document_key(p) for p in load_all_msgpack_l_gz(argv[1]))
        assert kept == kept_ref and all(n == 3 for n in kept.values())
        for field in ("documents", "against_documents", "too_short", "duplicate_keys", "dropped", "kept", "datapoints_read", "datapoints_kept",
                      "dropped_documents"):
            assert report[field] == want[field], field
        assert report["documents"] == 160 == report["kept"] + report["dropped"] and report["dropped"] > 0
        assert report["datapoints_kept"] == 3 * report["kept"] and len(report["dropped_documents"]) == report["dropped"]
        assert (report["duplicate_keys"] > 0) == bool(extra)
