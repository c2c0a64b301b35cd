from .count_penalty import count_penalty_logits_processor
from .dry import dry_logits_processor
from .logit_bias import make_logit_bias
from .repetition import make_repetition_penalty
from .token_automaton import TokenAutomaton, make_token_automaton
from .token_mask import check_vocab, make_token_mask, packed_token_mask, unpack_token_mask

repetition_penalty_logits_processor = make_repetition_penalty

__all__ = ["TokenAutomaton", "check_vocab", "count_penalty_logits_processor", "dry_logits_processor", "make_logit_bias", "make_repetition_penalty", "make_token_automaton", "make_token_mask", "packed_token_mask", "repetition_penalty_logits_processor",
           "unpack_token_mask"]
