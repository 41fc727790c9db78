"""The SGM forks (reference model_sgm_*): `sgm/model` is their drop-in `model` package -- the semantic-guidance head
that all eleven share, and model_sgm_2's encoder."""
