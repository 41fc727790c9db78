"""Drop-in replacement for the `model` package of model_sgm_mms_attach and model_sgm_mms_detach: `from model import
HTR_VT` and `from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch` resolve here when
`htr-vt_amd/sgm_mms` is first on sys.path ("The multi-mask SGM forks as a drop-in")."""
