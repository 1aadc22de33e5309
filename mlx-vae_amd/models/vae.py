"""ARCVAE on MI355X: encoder + decoder + separate sampling decoder (reference models/vae.py:8-131)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .decoder import MLXAutoregressiveDecoder
from .decoder_sampling import MLXAutoregressiveDecoderSampling
from .encoder import MLXEncoder


class ARCVAE:
    def __init__(self, vocab_size: int, embedding_dim: int = 256, hidden_dim: int = 512, latent_dim: int = 200,
                 num_conditions: int = 6, num_layers: int = 3, dropout: float = 0.2, device=None, generator=None):
        kw = dict(vocab_size=vocab_size, embedding_dim=embedding_dim, hidden_dim=hidden_dim, latent_dim=latent_dim,
                  num_conditions=num_conditions, num_layers=num_layers, device=device, generator=generator)
        self.encoder = MLXEncoder(dropout=dropout, **kw)
        self.decoder = MLXAutoregressiveDecoder(**kw)
        self.decoder_sampling = MLXAutoregressiveDecoderSampling(**kw)  # own weights (Q9)
        self.latent_dim = latent_dim

    def __call__(self, x, conditions, target_seq=None, teacher_forcing_ratio: float = 0.5,
                 eps: Optional[torch.Tensor] = None, coins: Optional[Sequence[bool]] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(recon_logits [B,T,V], mu, logvar, z)  (models/vae.py:63-99).  With target_seq=None the decoder
        free-runs for its default max_length=80 steps, as in the reference."""
        mu, logvar = self.encoder(x, conditions)
        z = self.encoder.reparameterize(mu, logvar, eps=eps)
        logits = self.decoder(z, conditions, target_seq=target_seq, teacher_forcing_ratio=teacher_forcing_ratio,
                              coins=coins)
        return logits, mu, logvar, z

    def generate(self, batch_size: int, conditions, max_length: int = 80, temperature: float = 1.0, *, sample: bool = False,
                 seed: int = 0, beam_width: Optional[int] = None, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, exact: bool = False, num_best: Optional[int] = None,
                 length_penalty=None, num_samples: Optional[int] = None, min_p: Optional[float] = None,
                 typical_p: Optional[float] = None, min_length: int = 0, num_draws: Optional[int] = None) -> torch.Tensor:
        """models/vae.py:101-131: z ~ N(0,I) (unused downstream, Q2) -> greedy sampler.  sample / seed (keyword-only extension):
        true categorical sampling instead of the reference's argmax, see MLXAutoregressiveDecoderSampling.  beam_width
        (keyword-only extension): the best hypothesis of a beam search of that width, [B, L] (generate_beam, early stopping).
        top_k / top_p (keyword-only extension, with sample=True): top-k / nucleus truncated sampling.  exact=True (keyword-only
        extension): the most probable sequence of every row, [B, L] (generate_map: exact, where beam search is a heuristic);
        exclusive with sample, beam_width, top_k and top_p.  num_best=K (keyword-only extension, with exact=True): the K most
        probable sequences of every row, [B, K, L], best first (generate_kbest: exact, where a K-wide beam is a heuristic).
        length_penalty (keyword-only extension, with exact=True): the exact optimum (or K best) of log-probability / n ** alpha,
        or max_length divisors -- see generate_map; tokens only, as without it.  num_samples=K (keyword-only extension, with
        sample=True): K DISTINCT random sequences of every row, [B, K, L] -- a sample without replacement
        (generate_without_replacement, seeded by `seed`); exclusive with beam_width, exact, top_k and top_p.  min_p / typical_p /
        min_length (keyword-only extension, with sample=True): min-p and locally typical truncation and the minimum-length mask of
        the end token, see generate_with_temperature; exclusive with beam_width, exact and num_samples.  num_draws=N (keyword-only
        extension, with sample=True): N INDEPENDENT random sequences of every condition row, [B, N, L], pad_token after each one's
        end (generate_many, seeded by `seed`) -- i.i.d. draws from the measure the list walk samples, combined with top_k, top_p,
        min_p, typical_p and min_length as there; exclusive with beam_width, exact, num_best, num_samples (the sampler WITHOUT
        replacement) and length_penalty.  For N molecules at one property target pass ONE condition row and num_draws=N, not N
        repeated rows: the table is then computed once.  The rows are those of `conditions`; batch_size is not used on this path."""
        trunc = min_p is not None or typical_p is not None or min_length != 0
        if num_draws is not None:
            if not sample:
                raise ValueError("num_draws needs sample=True")
            if exact or beam_width is not None or num_best is not None or num_samples is not None or length_penalty is not None:
                raise ValueError("num_draws is exclusive with beam_width, exact, num_best, num_samples and length_penalty")
            return self.decoder_sampling.generate_many(conditions, num_draws, max_length=max_length, temperature=temperature,
                                                       seed=seed, top_k=top_k, top_p=top_p, min_p=min_p, typical_p=typical_p,
                                                       min_length=min_length)[0]
        dev = self.decoder_sampling.decoder.store.device
        z = torch.randn(batch_size, self.latent_dim, device=dev)
        if num_samples is not None:
            if not sample:
                raise ValueError("num_samples needs sample=True")
            if exact or beam_width is not None or top_k is not None or top_p is not None or trunc:
                raise ValueError("num_samples is exclusive with beam_width, exact, top_k, top_p, min_p, typical_p and min_length")
            return self.decoder_sampling.generate_without_replacement(z, conditions, max_length=max_length, num_samples=num_samples,
                                                                      temperature=temperature, seed=seed)[0]
        if num_best is not None and not exact:
            raise ValueError("num_best needs exact=True")
        if length_penalty is not None and not exact:
            raise ValueError("length_penalty needs exact=True")
        if exact:
            if sample or beam_width is not None or top_k is not None or top_p is not None or trunc:
                raise ValueError("exact=True is exclusive with sample, beam_width, top_k, top_p, min_p, typical_p and min_length")
            if num_best is not None:
                return self.decoder_sampling.generate_kbest(z, conditions, max_length=max_length, num_best=num_best,
                                                            temperature=temperature, length_penalty=length_penalty)[0]
            return self.decoder_sampling.generate_map(z, conditions, max_length=max_length, temperature=temperature,
                                                      length_penalty=length_penalty)[0]
        if beam_width is not None:
            if sample:
                raise ValueError("beam_width and sample=True are exclusive")
            if top_k is not None or top_p is not None or trunc:
                raise ValueError("top_k / top_p / min_p / typical_p / min_length do not apply to beam search")
            tokens, _ = self.decoder_sampling.generate_beam(z, conditions, max_length=max_length, beam_width=beam_width,
                                                            temperature=temperature)
            best = tokens[:, 0, :]
            ended = best == self.decoder_sampling.end_token          # cut where every row's best hypothesis has ended
            length = torch.where(ended.any(1), ended.int().argmax(1) + 1, best.shape[1])
            return best[:, :int(length.max().item())].contiguous()
        return self.decoder_sampling.generate_with_temperature(z, conditions, max_length=max_length,
                                                               temperature=temperature, sample=sample, seed=seed,
                                                               top_k=top_k, top_p=top_p, min_p=min_p, typical_p=typical_p,
                                                               min_length=min_length)

    def parameters(self):
        return {"encoder": self.encoder.parameters(), "decoder": self.decoder.parameters(),
                "decoder_sampling": self.decoder_sampling.parameters()}
