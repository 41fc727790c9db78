"""The window-attention fork (reference model_window/): `window/model` is its drop-in `model` package."""
