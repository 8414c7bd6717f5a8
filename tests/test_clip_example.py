"""CPU: ``clip_example.interpret`` keeps the reference's name and signature (CLIP/example.py:8)."""
import inspect


def test_interpret_signature_is_the_references():
    from transformer_mm_explainability_amd import clip_example
    sig = inspect.signature(clip_example.interpret)
    assert str(sig) == "(image, text, model, device, index=None)"
    assert [p.name for p in sig.parameters.values()] == ["image", "text", "model", "device", "index"]
    assert sig.parameters["index"].default is None
