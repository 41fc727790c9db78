"""The local-global-parallel (LGP) fork (reference model_lgp/): `lgp/model` is its drop-in `model` package."""
