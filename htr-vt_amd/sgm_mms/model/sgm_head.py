"""The fork's sgm_head.py is the one all SGM forks share: the head of htrvt_amd.sgm, re-exported."""
from htrvt_amd.sgm.model.sgm_head import (SPECIAL_TOKENS, SGMHead, build_sgm_vocab, make_context_batch,  # noqa: F401
                                          texts_to_ids)
