"""Drop-in replacement for the LGP fork's `model` package (model_lgp/model/): `from model import HTR_VT` and
`from model.plg import LocalGlobalParallelBlockSimple` resolve here when `htr-vt_amd/lgp` is first on sys.path (see
INTEGRATION.md, "The LGP fork as a drop-in")."""
