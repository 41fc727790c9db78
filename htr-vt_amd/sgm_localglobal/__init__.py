"""The SGM local-global fork (reference model_sgm_localglobal/): `sgm_localglobal/model` is its drop-in `model` package."""
