"""Drop-in replacement for the SGM local-global fork's `model` package (model_sgm_localglobal/model/): `from model import
HTR_VT` and `from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch` resolve here when
`htr-vt_amd/sgm_localglobal` is first on sys.path ("The SGM local-global fork as a drop-in")."""
