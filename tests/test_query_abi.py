"""CPU: the table-query entry points exist at the ABI boundary (kc_lookup_device, kc_lookup,
kc_histogram) and the host helper that feeds them, encode_kmers, inverts decode_records."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import LIB, REPO
import kaarme_amd as ka

QUERY_SYMBOLS = ("kc_lookup_device", "kc_lookup", "kc_histogram")


def test_library_exports_query_symbols():
    lib = ctypes.CDLL(LIB)
    for name in QUERY_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_query_entry_points():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        text = f.read()
    for name in QUERY_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*" % name, text), name
    assert re.search(r"#define\s+KC_KEYS_DUMP\s+0\b", text)
    assert re.search(r"#define\s+KC_KEYS_TABLE\s+1\b", text)
    assert (ka.KEYS_DUMP, ka.KEYS_TABLE) == (0, 1)


@pytest.mark.parametrize("k", [1, 5, 31, 32, 33, 64, 127, 479])
def test_encode_kmers_inverts_decode_records(k):
    rng = np.random.default_rng(k)
    strings = ["".join(rng.choice(list("ACGT"), size=k)) for _ in range(50)]
    strings += ["A" * k, "T" * k, "C" * k, "G" * k]
    W = ka.words_for_k(k)
    keys = ka.encode_kmers(strings, k)
    assert keys.shape == (len(strings), W) and keys.dtype == np.uint64
    recs = np.concatenate([keys, np.arange(len(strings), dtype=np.uint64)[:, None]], axis=1)
    assert ka.decode_records(recs, k) == [(s, i) for i, s in enumerate(strings)]
    assert (ka.encode_kmers([s.lower() for s in strings], k) == keys).all()
    # no bit above 2k - 1
    top = 2 * k - 64 * (W - 1)
    assert not (keys[:, 0] >> np.uint64(top)).any()


def test_encode_kmers_rejects_other_characters():
    with pytest.raises(ValueError):
        ka.encode_kmers(["ACGTN"], 5)
    with pytest.raises(ValueError):
        ka.encode_kmers(["ACGT"], 5)
    assert ka.encode_kmers([], 31).shape == (0, 1)
