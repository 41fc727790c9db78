"""The multi-mask SGM forks model_sgm_mms_attach / model_sgm_mms_detach (identical `model/` directories):
`sgm_mms/model` is their drop-in `model` package."""
