#!/usr/bin/env python3
"""GPU tokenizer (K1) at the bench batch: 1024 rows of 150 synthetic words, S = 128; best of
event-timed rounds of back-to-back launches. One JSON line.

Default: the hash kernel. ``--vocab N``: the WordPiece kernel on a deterministic N-entry
generated vocabulary (``make_wordpiece_vocab``), same rows."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def main() -> int:
    from agent_tpu_amd import ops
    from agent_tpu_amd import tokenizer as T
    from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=0, help="time the WordPiece kernel on an N-entry generated vocabulary")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = a.rows
    text, offs = T.pack_rows(make_text_rows(rows, 150, seed=11))
    t = torch.from_numpy(text).to(dev)
    o = torch.from_numpy(offs).to(dev)
    out = {"kernel": "tokenize", "rows": rows, "bytes": int(text.size)}
    if a.vocab:
        vocab = T.WordPieceVocab([e.encode() for e in make_wordpiece_vocab(a.vocab, seed=0)])
        ids = torch.empty((rows, 128), dtype=torch.int32, device=dev)
        lens = torch.empty(rows, dtype=torch.int32, device=dev)

        def launch():
            ops.tokenize_wordpiece(t, o, 128, vocab, 2048, ids=ids, lens=lens)

        launch()
        torch.cuda.synchronize()
        out.update(kernel="tokenize_wordpiece", vocab=a.vocab, table_bytes=vocab.table_bytes,
                   tokens=int(lens.sum().item()) - 2 * rows, unk=int((ids == vocab.unk_id).sum().item()))
    else:
        def launch():
            ops.tokenize(t, o, 128, 30522, 2048)

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000.0 / 50)
    out["us_best"] = round(best, 1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
