"""Shared by the caption perturbation suites (CPU and ``-m gpu``): the plain-loop restatement of ``mmx_perturb_tokens``'s rule
(include/mmx_relevancy.h) and the two input sets of the evaluator tests.  No test lives here."""
import json
import math

import torch

TINY_LENGTHS = (2, 3, 4, 7, 11, 12)
CTX77_LENGTHS = (2, 3, 9, 17, 18, 33, 49, 65, 66, 77)
CTX77_CFG = dict(embed_dim=64, image_resolution=32, vision_layers=2, vision_width=64, vision_patch_size=16, context_length=77,
                 vocab_size=96, transformer_width=64, transformer_heads=2, transformer_layers=3)


def _key(x):
    """Total order of ``torch.sort(descending=True)``: NaN above +inf, +0.0 == -0.0."""
    return (1, 0.0) if math.isnan(x) else (0, x)


def restate(ids, scores, counts):
    """``ids [B, N]`` long, ``scores [B, N]`` fp32 (already negated for the positive test), ``counts [S][N - 1]`` ->
    ``(out_ids [S, B, N], out_eot [S, B], ranks [B, N])`` by the rule of the header, one caption and one step at a time."""
    B, N = ids.shape
    S = len(counts)
    out_ids = torch.zeros(S, B, N, dtype=torch.long)
    out_eot = torch.zeros(S, B, dtype=torch.long)
    ranks = torch.full((B, N), -1, dtype=torch.int32)
    for b in range(B):
        row, sc = ids[b].tolist(), scores[b].tolist()
        e = row.index(max(row))                                  # the first maximum: text.argmax(dim=-1)
        words = list(range(1, e))
        W = max(e - 1, 0)
        rank, key = {}, [_key(x) for x in sc]
        for p in words:
            rank[p] = sum(1 for j in words if key[j] > key[p] or (key[j] == key[p] and j < p))
            ranks[b, p] = rank[p]
        for s in range(S):
            kept = [p for p in words if rank[p] < counts[s][W]]
            new = [row[0]] + [row[p] for p in kept] + ([row[e]] if e > 0 else [])
            out_ids[s, b, :len(new)] = torch.tensor(new)
            out_eot[s, b] = len(new) - 1
    return out_ids, out_eot, ranks


def captions(lengths, context, vocab, generator):
    """SOT is ``vocab - 2``, the words ``randint(1, vocab - 2)``, EOT ``vocab - 1`` (the arg-max), zeros after."""
    texts = torch.zeros(len(lengths), context, dtype=torch.long)
    for b, n in enumerate(lengths):
        texts[b, 0] = vocab - 2
        texts[b, 1:n - 1] = torch.randint(1, vocab - 2, (n - 2,), generator=generator)
        texts[b, n - 1] = vocab - 1
    return texts


def evaluator_inputs(cfg, lengths, seed_images, seed_texts, n_images=5):
    """``(images [5, 3, R, R], cam [B, ctx], texts [B, ctx])``: first ``randn`` for the images, then ``rand(B, ctx)`` from one
    generator; the caption ids from a second one."""
    g = torch.Generator().manual_seed(seed_images)
    res, ctx = cfg["image_resolution"], cfg["context_length"]
    images = torch.randn(n_images, 3, res, res, generator=g)
    cam = torch.rand(len(lengths), ctx, generator=g)
    texts = captions(lengths, ctx, cfg["vocab_size"], torch.Generator().manual_seed(seed_texts))
    return images, cam, texts


def tiny_cfg(golden):
    return json.loads(str(golden("clip_tiny")["cfg_json"]))
