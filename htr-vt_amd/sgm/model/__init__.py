"""Drop-in replacement for the SGM forks' `model` package (model_sgm_2/model/): `from model import HTR_VT` and
`from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch` resolve here when `htr-vt_amd/sgm` is first on
sys.path."""
