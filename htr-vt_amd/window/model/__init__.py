"""Drop-in replacement for the window-attention fork's `model` package (model_window/model/): `from model import HTR_VT`
resolves here when `htr-vt_amd/window` is first on sys.path."""
