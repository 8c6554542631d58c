"""Device-resident token-vector indexes for ``map_maxsim``.

An index is two local ``.npy`` files. The tokens file is a 2-D C-order ``[T, P]`` array of ``float16`` or
``float32``: the unit token vectors of all passages back to back, live tokens only ([CLS] and [SEP] included),
no padding rows. The offsets file, the tokens file's name with ``.npy`` replaced by ``.offsets.npy``, is a 1-D
``int64`` ``[N + 1]``: ``off[0] = 0``, strictly increasing, ``off[N] = T``; passage ``p`` is rows
``off[p] .. off[p + 1] - 1``.

:func:`load_index` is modelled on :func:`runtime.search.load_corpus`: both files are memory-mapped, a DP rank
reads only the token rows ``off[start] .. off[start + count]`` of its contiguous share of the passages, the
offsets are rebased to the slice, and the slice stays on the device as stored (fp16 stays fp16) in
``runtime.search``'s LRU under a key of its own kind, ``(path, mtime, size, offsets mtime, offsets size, start,
count, device, "maxsim")``: a rewritten file misses. :func:`write_index` writes both files atomically.
"""
from __future__ import annotations

import os
from typing import Any, Dict, NamedTuple, Tuple

import torch

from . import search as rs

#: the loader's and writer's input errors (``ops/map_maxsim.py`` lists them in ``INDEX_ERRORS``)
ERRORS: Dict[str, str] = {
    "index_file": "index_uri must be a local 2-D float32 or float16 .npy file of token vectors",
    "offsets_file": "index offsets must be a local 1-D int64 .npy file next to index_uri (<name>.offsets.npy), "
                    "starting at 0, strictly increasing and ending at the token count",
    "index_nonfinite": "index holds non-finite values",
    "index_too_large": "index slice exceeds SEARCH_INDEX_MAX_GB",
}
DTYPES = ("float16", "float32")


class TokenIndex(NamedTuple):
    tokens: torch.Tensor  # [T_r, P] fp16 or fp32 on the device, contiguous: the slice's token rows
    offsets: torch.Tensor  # [count + 1] int64 on the device, rebased: offsets[0] == 0
    start: int  # passage of the file that slice passage 0 is
    total: int  # passages of the whole file
    dtype: str  # "float16" or "float32", as stored
    cached: bool  # served from the LRU

    @property
    def count(self) -> int:
        return int(self.offsets.numel()) - 1


def offsets_path(path: str) -> str:
    return (path[:-len(".npy")] if path.endswith(".npy") else path) + ".offsets.npy"


def open_index(uri: Any):
    """-> (tokens memmap, offsets memmap, realpath, stat, offsets stat); shapes and dtypes checked, only the
    first and last offset read."""
    import numpy as np

    try:
        path = os.path.realpath(rs.local_path(uri))
        st = os.stat(path)
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        raise ValueError(ERRORS["index_file"]) from None
    if not isinstance(arr, np.ndarray) or arr.ndim != 2 or arr.dtype.str not in ("<f4", "<f2") \
            or not arr.flags["C_CONTIGUOUS"] or arr.shape[0] == 0 or arr.shape[1] == 0:
        raise ValueError(ERRORS["index_file"])
    try:
        opath = offsets_path(path)
        ost = os.stat(opath)
        off = np.load(opath, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        raise ValueError(ERRORS["offsets_file"]) from None
    if not isinstance(off, np.ndarray) or off.ndim != 1 or off.dtype.str != "<i8" or off.shape[0] < 2 \
            or int(off[0]) != 0 or int(off[-1]) != int(arr.shape[0]):
        raise ValueError(ERRORS["offsets_file"])
    return arr, off, path, st, ost


def index_shape(uri: Any) -> Tuple[int, int, int, str]:
    """``(passages, tokens, width, dtype)`` of the files."""
    arr, off, _, _, _ = open_index(uri)
    return int(off.shape[0]) - 1, int(arr.shape[0]), int(arr.shape[1]), "float16" if arr.dtype.str == "<f2" else "float32"


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu")) -> TokenIndex:
    """Passages ``[start, start + count)`` (``count < 0``: to the end) of the index on ``device``."""
    import numpy as np

    arr, off, path, st, ost = open_index(uri)
    total, dim = int(off.shape[0]) - 1, int(arr.shape[1])
    dtype = "float16" if arr.dtype.str == "<f2" else "float32"
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, ost.st_mtime_ns, ost.st_size, start, count, str(device), "maxsim")
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return TokenIndex(hit[0], hit[1], start, total, dtype, True)
    o = np.array(off[start:start + count + 1], dtype=np.int64, order="C")  # only this slice is read
    if o.size and (bool((np.diff(o) <= 0).any()) or int(o[0]) < 0 or int(o[-1]) > int(arr.shape[0])):
        raise ValueError(ERRORS["offsets_file"])
    r0, r1 = (int(o[0]), int(o[-1])) if count else (0, 0)
    if (r1 - r0) * dim * arr.dtype.itemsize + o.size * 8 > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["index_too_large"])
    tok = torch.empty((r1 - r0, dim), dtype=torch.float16 if dtype == "float16" else torch.float32, device=device)
    rows = max(1, rs.CHUNK_BYTES // (dim * 4))
    for lo in range(r0, r1, rows):  # in row chunks, as the fp16 corpus loader
        hi = min(lo + rows, r1)
        part = torch.from_numpy(np.array(arr[lo:hi], order="C")).to(device)
        if not bool(torch.isfinite(part).all()):
            raise ValueError(ERRORS["index_nonfinite"])
        tok[lo - r0:hi - r0] = part
    offs = torch.from_numpy(o - r0).to(device).contiguous()
    with rs._lock:
        rs._cache[key] = (tok, offs)
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return TokenIndex(tok, offs, start, total, dtype, False)


def _write_npy(path: str, arr) -> None:
    import numpy as np

    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            np.save(f, arr, allow_pickle=False)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


def write_index(uri: Any, tok: torch.Tensor, lens: torch.Tensor, dtype: str = "float16") -> Dict[str, Any]:
    """Writes the packed fp32 rows ``tok [T, P]`` of passages with ``lens [N]`` tokens as an index of ``dtype``
    (fp16: round to nearest): each file through a temporary file and ``os.replace``, the offsets first, so a
    reader that finds the new tokens file finds its offsets."""
    import numpy as np

    if dtype not in DTYPES:
        raise ValueError("write_index: dtype must be 'float16' or 'float32'")
    path = rs.local_path(uri)
    off = np.zeros(int(lens.numel()) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens.cpu().numpy().astype(np.int64))
    if int(off[-1]) != int(tok.shape[0]):
        raise ValueError("write_index: lens must sum to the token rows")
    rows = tok.detach().cpu().to(torch.float16 if dtype == "float16" else torch.float32).contiguous().numpy()
    _write_npy(offsets_path(path), off)
    _write_npy(path, rows)
    return {"index_uri": path, "offsets_uri": offsets_path(path), "passage_count": int(lens.numel()),
            "token_count": int(tok.shape[0]), "dim": int(tok.shape[1]), "dtype": dtype,
            "bytes": int(os.path.getsize(path) + os.path.getsize(offsets_path(path)))}
