"""The reference's own results for the tests that compare against it, so that they stand without its sources: computed live by
oracle/_ref (the reference's code compiled in place) where that library is built, read back from tests/golden/reference/<key>.npz
otherwise. `SS_RECORD_REFERENCE=1 python -m pytest tests -m "not gpu"` on a machine with the reference's sources writes the records.

A result is a dict of arrays and of lists of arrays (one per frame). Arrays larger than DIGEST_ABOVE bytes are recorded as their
SHA-256 (the tests hold the restatement bit-exact to them); everything else is recorded as it is."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
DIGEST_ABOVE = 64 << 10


class Digest(str):
    """The SHA-256 of an array's dtype, shape and bytes, standing in for an array too large to record."""


def digest(a) -> Digest:
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return Digest(h.hexdigest())


def assert_same(got, want, err_msg=""):
    """Bit-exact: got equals the reference's array (or the digest recorded in its place)."""
    if isinstance(want, Digest):
        assert digest(got) == want, f"differs from the reference's recorded result {err_msg}"
    else:
        np.testing.assert_array_equal(got, want, err_msg=err_msg)


def _save(path, out: dict):
    arrays = {}
    for k, v in out.items():
        if isinstance(v, list):
            arrays[k + "__shapes"] = np.array([a.shape for a in v], np.int64).reshape(len(v), -1)
            arrays[k + "__cat"] = np.concatenate([np.asarray(a).reshape(-1) for a in v]) if v else np.zeros(0)
        elif np.asarray(v).nbytes > DIGEST_ABOVE:
            arrays[k + "__sha256"] = np.array(digest(v))
        else:
            arrays[k] = np.asarray(v)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **arrays)


def _load(path) -> dict:
    out = {}
    with np.load(path) as z:
        for name in z.files:
            if name.endswith("__sha256"):
                out[name[:-8]] = Digest(str(z[name]))
            elif name.endswith("__shapes"):
                k = name[:-8]
                shapes, cat = z[name], z[k + "__cat"]
                items, pos = [], 0
                for s in shapes:
                    size = int(np.prod(s))
                    items.append(cat[pos:pos + size].reshape(tuple(int(d) for d in s)))
                    pos += size
                out[k] = items
            elif not name.endswith("__cat"):
                out[name] = z[name]
    return out


def reference(oracle_mod, key: str, compute, keep=None) -> dict:
    """compute() runs the reference (oracle_mod.ref() / RefChain) and returns its result; `keep` names the entries to record
    (all by default). Live where oracle/_ref is built, recorded otherwise."""
    path = os.path.join(GOLDEN, key + ".npz")
    if oracle_mod.have_ref():
        out = compute()
        out = {k: out[k] for k in (keep or out)}
        if os.environ.get("SS_RECORD_REFERENCE"):
            _save(path, out)
        return out
    if not os.path.exists(path):
        pytest.fail(f"oracle/_ref is not built and {os.path.relpath(path)} is not recorded")
    return _load(path)
