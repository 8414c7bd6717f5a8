"""``interpret`` of CLIP/example.py:8-32 under the reference's name: one image, C text prompts, explains
``logits_per_image[0, index]`` and returns ``image_relevance [Ni-1]`` (the reference also plots; this does not).

The notebook-style ``interpret`` (cell 6: one image repeated over B texts, both towers) lives in ``clip_explainability``;
many images at once: ``clip_explainability.interpret_batch``.
"""
from __future__ import annotations

from .clip_explainability import interpret_single


def interpret(image, text, model, device, index=None):
    """CLIP/example.py:8 ``interpret(image, text, model, device, index=None)`` without the plotting."""
    return interpret_single(image, text, model, device, index=index)
