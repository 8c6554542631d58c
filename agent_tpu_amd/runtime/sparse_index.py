"""Resident inverted indexes for ``map_sparse_search``: a CSR ``.npz`` of term weights -> ``ops.SparseIndex``.

**File.** The arrays of ``scipy.sparse.save_npz`` for a CSR matrix: ``indptr`` (int32 or int64 ``[rows + 1]``),
``indices`` (int32 or int64 token ids), ``data`` (fp32 weights), ``shape`` (``[rows, vocabulary]``) and ``format``
(``b"csr"``). It is read with numpy alone (``allow_pickle=False``); scipy is not needed. ``map_sparse_embed`` with
``output: "npz"`` writes it (:func:`save_csr`).

**Reading.** The rows, the vocabulary and the count of entries come from the .npy headers inside the archive and are
kept per (path, mtime, size): a job that finds its index in the cache reads nothing else. On a miss the three arrays
are memory-mapped in place where the archive stores them uncompressed (``numpy.savez``, which :func:`save_csr` uses),
so only the ranges of the rank's slice are read; a compressed member (``scipy.sparse.save_npz``'s default) is
decompressed whole.

**Build.** The slice streams to the device by groups of ``GROUP_BLOCKS`` blocks of 8192 rows; each group is checked
and built (``ops.sparse_index_build``) and the groups are joined (``ops.sparse_index_cat``), so the forward (CSR) form
is never resident on the device beyond one group. The checks of a group synchronise with the host and sort the
group's ``row * V + token`` keys (the distinctness check): about three times the group's CSR in device memory for
the moment.

**Cache.** The entry lives in ``runtime.search``'s LRU under the file's key extended by ``("sparse",)``.
"""
from __future__ import annotations

import os
from typing import Any, Dict, NamedTuple, Tuple

import torch

from . import search as rs

GROUP_BLOCKS = 16

#: the loader's input errors (``ops/map_sparse_search.py`` lists them in its ``ERRORS``)
ERRORS: Dict[str, str] = {
    "corpus_file": "payload.corpus_uri must be a local .npz file holding a CSR matrix (indptr, indices, data, shape, "
                   "format) with float32 data",
    "corpus_values": "corpus rows must have at most 1024 distinct token ids inside the vocabulary and finite "
                     "weights in (0, 256]",
    "corpus_empty": "corpus has no rows",
    "sparse_too_large": "sparse corpus slice exceeds SEARCH_INDEX_MAX_GB of postings",
}


class ResidentIndex(NamedTuple):
    index: Any  # ops.SparseIndex of the slice, or None for an empty slice
    rows: int  # rows of the slice
    start: int  # row of the file that slice row 0 is
    total: int  # rows of the whole file
    vocab: int
    nnz: int  # stored entries of the whole file
    cached: bool = False


def save_csr(path: str, indptr, indices, data, shape: Tuple[int, int]) -> None:
    """Write the file above (uncompressed) to a temporary name, then ``os.replace`` it into place."""
    import numpy as np

    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, "wb") as f:
        np.savez(f, indptr=np.asarray(indptr, dtype=np.int64), indices=np.asarray(indices, dtype=np.int32),
                 data=np.asarray(data, dtype=np.float32), shape=np.asarray(shape, dtype=np.int64),
                 format=np.array(b"csr"))
    os.replace(tmp, path)


_meta: Dict[Tuple, Tuple[int, int, int]] = {}  # (path, mtime, size) -> (rows, vocabulary, nnz): a few entries


def _member(zf, path: str, name: str, load: bool):
    """One array of the archive: its (shape, dtype) from the .npy header alone, or with ``load`` the array itself:
    a memory map of the file where the member is stored uncompressed (``numpy.savez``), so that only the ranges
    a build touches are read, or the decompressed member (``scipy.sparse.save_npz``'s default)."""
    import struct
    import zipfile

    import numpy as np
    from numpy.lib import format as npf

    info = zf.getinfo(name + ".npy")
    with zf.open(info) as f:
        version = npf.read_magic(f)
        shape, fortran, dtype = (npf.read_array_header_1_0 if version == (1, 0) else npf.read_array_header_2_0)(f)
        skip = f.tell()
        if dtype.hasobject or (fortran and len(shape) > 1):
            raise ValueError(name)
        if not load:
            return shape, dtype
        if info.compress_type != zipfile.ZIP_STORED:
            return np.frombuffer(f.read(), dtype=dtype).reshape(shape)
    with open(path, "rb") as raw:  # the local file header: 30 bytes, then the name and the extra field
        raw.seek(info.header_offset + 26)
        n_name, n_extra = struct.unpack("<HH", raw.read(4))
    return np.memmap(path, dtype=dtype, mode="r", offset=info.header_offset + 30 + n_name + n_extra + skip, shape=shape)


def corpus_meta(uri: Any) -> Tuple[int, int, int, str, Any]:
    """-> (rows, vocabulary, stored entries, realpath, stat) from the archive's headers and its two tiny arrays; the
    structure is checked, ``indptr`` / ``indices`` / ``data`` are not read. Kept per (path, mtime, size)."""
    import zipfile

    try:
        path = os.path.realpath(rs.local_path(uri))
        st = os.stat(path)
        key = (path, st.st_mtime_ns, st.st_size)
        if key not in _meta:
            with zipfile.ZipFile(path) as zf:
                fmt, shape = _member(zf, path, "format", True), _member(zf, path, "shape", True)
                heads = [_member(zf, path, n, False) for n in ("indptr", "indices", "data")]
            (ps, pt), (ts, tt), (ds, dt) = heads
            if not (bytes(fmt.item() if fmt.dtype.kind == "S" else str(fmt.item()).encode()) == b"csr"
                    and shape.shape == (2,) and len(ps) == len(ts) == len(ds) == 1 and pt.kind == "i" and tt.kind == "i"
                    and dt == "float32" and ps[0] == int(shape[0]) + 1 and ts == ds and 1 <= int(shape[1]) < 2 ** 31 - 1):
                raise ValueError("structure")
            while len(_meta) >= 16:
                _meta.pop(next(iter(_meta)))
            _meta[key] = (int(shape[0]), int(shape[1]), int(ts[0]))
    except Exception:
        raise ValueError(ERRORS["corpus_file"]) from None
    return _meta[key] + (path, st)


def _arrays(path: str, nnz: int):
    """(indptr, indices, data) of the archive for a build: memory maps where the members are stored."""
    import zipfile

    try:
        with zipfile.ZipFile(path) as zf:
            indptr, indices, data = (_member(zf, path, n, True) for n in ("indptr", "indices", "data"))
        if int(indptr[0]) != 0 or int(indptr[-1]) != nnz:
            raise ValueError("indptr")
    except Exception:
        raise ValueError(ERRORS["corpus_file"]) from None
    return indptr, indices, data


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu")) -> ResidentIndex:
    """The cached index of rows ``[start, start + count)`` (``count < 0``: to the end) of the file, or a fresh build.
    A cache hit reads the archive's headers at most (:func:`corpus_meta`); a build reads the slice's ranges of the
    three arrays, group by group. No collective."""
    import numpy as np

    from .. import ops
    from ..ops.sparse_index import BLOCK_ROWS

    total, V, nnz, path, st = corpus_meta(uri)
    if total == 0:
        raise ValueError(ERRORS["corpus_empty"])
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, str(device), "sparse")
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return ResidentIndex(ops.SparseIndex(*hit), count, start, total, V, nnz, True)
    if count == 0:
        return ResidentIndex(None, 0, start, total, V, nnz, False)
    indptr, indices, data = _arrays(path, nnz)
    lo, hi = int(indptr[start]), int(indptr[start + count])
    if 4 * (hi - lo) + 4 * (V + 1) * -(-count // BLOCK_ROWS) > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["sparse_too_large"])
    parts, step = [], GROUP_BLOCKS * BLOCK_ROWS
    try:
        for a in range(start, start + count, step):
            b = min(a + step, start + count)
            ptr = np.asarray(indptr[a:b + 1], dtype=np.int64)  # copies: only this group's ranges are read
            ea, eb = int(ptr[0]), int(ptr[-1])
            if np.any(ptr[1:] < ptr[:-1]) or not lo <= ea <= eb <= hi:
                raise ValueError("indptr")
            tok = np.asarray(indices[ea:eb])
            if tok.size and (int(tok.min()) < 0 or int(tok.max()) >= V):  # before the cast to int32
                raise ValueError("indices")
            parts.append(ops.sparse_index_build(torch.from_numpy(ptr - ea).to(device),
                                                torch.from_numpy(tok.astype(np.int32)).to(device),
                                                torch.from_numpy(np.array(data[ea:eb], dtype=np.float32)).to(device), V))
    except ValueError:
        raise ValueError(ERRORS["corpus_values"]) from None
    index = ops.sparse_index_cat(parts)
    with rs._lock:
        rs._cache[key] = tuple(index)  # three tensors and two scalars: cache_info counts the tensors
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return ResidentIndex(index, count, start, total, V, nnz, False)


def search(res: ResidentIndex, q_ptr: torch.Tensor, q_tok: torch.Tensor, q_w: torch.Tensor, k: int, id_base: int = 0
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ops.sparse_scan_topk`` over the slice on the queries' device: (scores ``[nq, k]``, ids ``[nq, k]``, counts),
    padded with ``(-inf, 2^62)``. An empty slice (a DP rank beyond the corpus) gives padding only."""
    from .. import ops
    from ..ops.sparse_index import _padding

    if res.index is None:
        return _padding(int(q_ptr.numel()) - 1, k, q_tok.device)
    return ops.sparse_scan_topk(res.index, q_ptr, q_tok, q_w, k, id_base)
