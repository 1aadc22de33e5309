"""MLXAutoregressiveDecoderSampling on MI355X (reference models/decoder_sampling.py:6-129).

Owns its OWN, never-trained decoder (Q9: not weight-shared with ARCVAE.decoder); "temperature
sampling" is argmax(softmax(logits / T)) = greedy; tokens after EOS are still generated; with
early stopping the output is cut where every row has emitted EOS.  One dense decoder pass
(B*V rows) + one table walk replaces the reference's max_length dependent steps and its per-step
host sync; `load_from_decoder` is an explicit extension to sample from trained weights, and `sample=True` the true categorical
sampling the reference marks TODO (decoder_sampling.py:115-116): an extension with no reference behaviour to match.  So is
`generate_beam` (beam search with scores, csrc/beam.hip); `decoder.sequence_log_prob` scores given sequences; and
`sample=True` with `top_k` / `top_p` (truncated sampling, csrc/sample.hip); and `generate_map` / `token_marginals` /
`length_distribution`: the exact most probable sequence and the exact per-step token and length distributions of the chain the
dense table defines (csrc/chain.hip); and `generate_kbest`: the exact K most probable sequences of that chain (csrc/kbest.hip)."""
from __future__ import annotations

import torch

from arcvae_hip import engine as E
from arcvae_hip._lib import call, ptr, stream_ptr
from arcvae_hip.module import as_f32

from .decoder import MLXAutoregressiveDecoder


class MLXAutoregressiveDecoderSampling:
    def __init__(self, vocab_size: int, embedding_dim: int = 256, hidden_dim: int = 512, latent_dim: int = 200,
                 num_conditions: int = 6, num_layers: int = 3, pad_token: int = 0, end_token: int = 2, device=None,
                 generator=None):
        self.decoder = MLXAutoregressiveDecoder(vocab_size, embedding_dim, hidden_dim, latent_dim, num_conditions,
                                                num_layers, pad_token, end_token, device=device, generator=generator)
        self.vocab_size, self.embedding_dim, self.hidden_dim = vocab_size, embedding_dim, hidden_dim
        self.latent_dim, self.num_conditions = latent_dim, num_conditions
        self.pad_token, self.end_token = pad_token, end_token
        self._graphs = {}

    def load_from_decoder(self, other: MLXAutoregressiveDecoder) -> None:
        """Extension (absent in the reference): copy trained decoder weights into the sampler."""
        self.decoder.store.flat.copy_(other.store.flat)

    def parameters(self):
        return {"decoder": self.decoder.parameters()}

    def generate_with_temperature(self, z, conditions, max_length: int = 80, temperature: float = 1.0,
                                  early_stopping: bool = True, use_graph: bool = True, *, sample: bool = False,
                                  seed: int = 0, top_k=None, top_p=None) -> torch.Tensor:
        """[B, t_stop] int32 tokens (models/decoder_sampling.py:48-128).  z is accepted and unused (Q2).
        sample=True (keyword-only extension; the default reproduces the reference's greedy "temperature sampling", Q9): every token is
        DRAWN from softmax(logits / temperature) -- what decoder_sampling.py:115-116 leaves as a TODO -- with a counter-based
        generator keyed by (seed, row, step): the same seed returns the same molecules.
        top_k / top_p (keyword-only extension, with sample=True): draw from the truncated distribution instead -- the top_k most
        likely tokens (ties to the lower token), then the smallest prefix of them holding top_p of their renormalised mass
        (include/arcvae_hip.h arcvae_dec_sample_chain_topkp).  None = no truncation of that kind; both None = the categorical path."""
        if top_k is not None or top_p is not None:
            if not sample:
                raise ValueError("top_k / top_p need sample=True")
            return self._generate_topkp(conditions, max_length, temperature, early_stopping, use_graph, int(seed), top_k, top_p)
        if sample:
            return self._generate_categorical(conditions, max_length, temperature, early_stopping, int(seed))
        dec = self.decoder
        dev = dec.store.device
        cond = as_f32(conditions, dev)
        B = cond.shape[0]
        ws = dec.workspace(B, max_length)
        ws.cond.copy_(cond.reshape(B, dec.num_conditions))
        key = (B, max_length, float(temperature))
        if key not in self._graphs:
            self._graphs[key] = dict(tokens=torch.zeros(B, max_length, dtype=torch.int32, device=dev),
                                     first_end=torch.zeros(B, dtype=torch.int32, device=dev), graph=None)
        st = self._graphs[key]

        def enqueue():
            E.decoder_forward_dense(dec.store, ws, dec.dims, mode=1, temperature=temperature, keep_gpre=False, alone=True)
            call("arcvae_dec_sample_chain", ptr(ws.nxt), ptr(st["tokens"]), ptr(st["first_end"]), B, dec.vocab_size,
                 max_length, dec.end_token, stream_ptr())

        if not use_graph:
            enqueue()
        elif st["graph"] is None:
            enqueue()  # first call runs eagerly, then the decode pass is captured for replay
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                enqueue()
            st["graph"] = g
        else:
            st["graph"].replay()
        tokens = st["tokens"]
        if early_stopping:
            # reference: the loop breaks at the first step t where every row has already ended, i.e. after
            # max_b(first EOS index) + 1 tokens; one host read replaces its per-step mx.all() sync
            t_stop = int(st["first_end"].max().item()) + 1
            tokens = tokens[:, :min(t_stop, max_length)]
        return tokens.clone()

    def _generate_categorical(self, conditions, max_length: int, temperature: float, early_stopping: bool, seed: int) -> torch.Tensor:
        """One dense decoder pass (raw logits of all B*V (row, token) pairs), then arcvae_dec_sample_chain_categorical: a wave per
        row walks start token -> sampled token -> ... through the table of distributions.  Eager launches (the seed is a launch
        argument; the greedy path's captured pass is untouched)."""
        import ctypes as C
        if not temperature > 0.0:
            raise ValueError("temperature must be > 0 for categorical sampling")
        dec = self.decoder
        dev = dec.store.device
        cond = as_f32(conditions, dev)
        B = cond.shape[0]
        ws = dec.workspace(B, max_length)
        ws.cond.copy_(cond.reshape(B, dec.num_conditions))
        tokens = torch.zeros(B, max_length, dtype=torch.int32, device=dev)
        first_end = torch.zeros(B, dtype=torch.int32, device=dev)
        E.decoder_forward_dense(dec.store, ws, dec.dims, mode=0, keep_gpre=False, alone=True)
        call("arcvae_dec_sample_chain_categorical", ptr(ws.logits), ptr(tokens), ptr(first_end), B, dec.vocab_size, max_length,
             dec.end_token, float(temperature), C.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), stream_ptr())
        if early_stopping:
            tokens = tokens[:, :min(int(first_end.max().item()) + 1, max_length)]
        return tokens.clone()

    def _generate_topkp(self, conditions, max_length: int, temperature: float, early_stopping: bool, use_graph: bool, seed: int,
                        top_k, top_p) -> torch.Tensor:
        """One dense decoder pass (mode 0: raw logits of all B*V (row, token) pairs), then arcvae_dec_sample_chain_topkp: a pre-pass
        truncates every table row once, and a wave per row walks start token -> drawn token -> ... through those lists.  The seed is
        read by the kernel from a device word written before the launch, so the pass is captured once per (B, max_length,
        temperature, top_k, top_p) and replayed for every seed; use_graph=False launches the same kernels eagerly."""
        import ctypes as C
        if not temperature > 0.0:
            raise ValueError("temperature must be > 0 for top-k / top-p sampling")
        k = 0 if top_k is None else int(top_k)
        if top_k is not None and k < 1:
            raise ValueError("top_k must be >= 1")
        p = 1.0 if top_p is None else float(top_p)
        if not 0.0 < p <= 1.0 or not 0.0 < float(C.c_float(p).value) <= 1.0:
            raise ValueError("top_p must lie in (0, 1]")
        dec = self.decoder
        if dec.vocab_size > 256:
            raise ValueError("top-k / top-p sampling needs vocab_size <= 256")
        dev = dec.store.device
        cond = as_f32(conditions, dev)
        B = cond.shape[0]
        ws = dec.workspace(B, max_length)
        ws.cond.copy_(cond.reshape(B, dec.num_conditions))
        key = ("topkp", B, max_length, float(temperature), k, p)
        if key not in self._graphs:
            nbytes = C.c_long(0)
            call("arcvae_dec_topkp_ws_bytes", B, dec.vocab_size, k, C.byref(nbytes))
            self._graphs[key] = dict(tokens=torch.zeros(B, max_length, dtype=torch.int32, device=dev),
                                     first_end=torch.zeros(B, dtype=torch.int32, device=dev),
                                     seed=torch.zeros(1, dtype=torch.int64, device=dev),
                                     scratch=torch.empty(nbytes.value, dtype=torch.uint8, device=dev), graph=None)
        st = self._graphs[key]
        s64 = seed & 0xFFFFFFFFFFFFFFFF
        st["seed"].fill_(s64 - (1 << 64) if s64 >= 1 << 63 else s64)       # the 64-bit word the kernel reads

        def enqueue():
            E.decoder_forward_dense(dec.store, ws, dec.dims, mode=0, keep_gpre=False, alone=True)
            call("arcvae_dec_sample_chain_topkp", ptr(ws.logits), ptr(st["tokens"]), ptr(st["first_end"]), ptr(st["scratch"]),
                 st["scratch"].numel(), B, dec.vocab_size, max_length, dec.end_token, float(temperature), k, p, ptr(st["seed"]),
                 stream_ptr())

        if not use_graph:
            enqueue()
        elif st["graph"] is None:
            enqueue()  # first call runs eagerly, then the decode pass is captured for replay
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                enqueue()
            st["graph"] = g
        else:
            st["graph"].replay()
        tokens = st["tokens"]
        if early_stopping:
            tokens = tokens[:, :min(int(st["first_end"].max().item()) + 1, max_length)]
        return tokens.clone()

    def generate_beam(self, z, conditions, max_length: int = 80, beam_width: int = 4, temperature: float = 1.0,
                      min_length: int = 0, early_stopping: bool = True):
        """Extension (absent in the reference): the beam_width most probable sequences per row under log_softmax(logits / T),
        found by beam search -> (tokens [B, K, L] int32, scores [B, K] float32, descending).  z is accepted and unused (Q2).
        Positions after a hypothesis' first end_token hold pad_token; end_token is not proposed before step min_length; ties
        are broken by parent slot, then token (the lower first).  A slot with no finite candidate (beam_width above what the
        vocabulary can fill) has score -inf and pad tokens.  early_stopping: L = the longest returned hypothesis (first EOS + 1,
        max_length without one); otherwise L = max_length.  Each score equals decoder.sequence_log_prob of its tokens."""
        import ctypes as C
        dec = self.decoder
        V = dec.vocab_size
        if not temperature > 0.0:
            raise ValueError("temperature must be > 0")
        if not 1 <= int(beam_width) <= 32:
            raise ValueError("beam_width must lie in [1, 32]")
        if int(max_length) < 1 or not 0 <= int(min_length) <= int(max_length):
            raise ValueError("need max_length >= 1 and 0 <= min_length <= max_length")
        if V > 256 or not 0 <= self.pad_token <= 255:
            raise ValueError("beam search needs vocab_size <= 256 and 0 <= pad_token <= 255")
        K, T = int(beam_width), int(max_length)
        dev = dec.store.device
        cond = as_f32(conditions, dev)
        B = cond.shape[0]
        ws = dec.workspace(B, T)
        ws.cond.copy_(cond.reshape(B, dec.num_conditions))
        nbytes = C.c_long(0)
        call("arcvae_dec_beam_ws_bytes", B, K, T, C.byref(nbytes))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        lse = torch.empty(B * V, dtype=torch.float32, device=dev)
        tokens = torch.empty(B, K, T, dtype=torch.int32, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
        E.decoder_forward_dense(dec.store, ws, dec.dims, mode=0, keep_gpre=False, alone=True)
        call("arcvae_dec_row_lse", ptr(ws.logits), ptr(lse), B * V, V, float(temperature), stream_ptr())
        call("arcvae_dec_beam_search", ptr(ws.logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch),
             nbytes.value, B, V, K, T, int(min_length), self.end_token, self.pad_token, float(temperature), stream_ptr())
        if early_stopping:
            tokens = tokens[:, :, :int(lengths.max().item())].contiguous()
        return tokens, scores

    def _chain_table(self, conditions, max_length: int, temperature: float):
        """The dense pass (mode 0) and the rows' lse for `conditions` -> (logits [B*V, V] in the workspace, lse [B*V], B)."""
        dec = self.decoder
        if not 0.0 < float(temperature) < float("inf"):
            raise ValueError("temperature must be finite and > 0")
        if int(max_length) < 1:
            raise ValueError("need max_length >= 1")
        if dec.vocab_size > 256 or not 0 <= self.end_token < dec.vocab_size:
            raise ValueError("needs vocab_size <= 256 and 0 <= end_token < vocab_size")
        dev = dec.store.device
        cond = as_f32(conditions, dev)
        B = cond.shape[0]
        ws = dec.workspace(B, int(max_length))
        ws.cond.copy_(cond.reshape(B, dec.num_conditions))
        lse = torch.empty(B * dec.vocab_size, dtype=torch.float32, device=dev)
        E.decoder_forward_dense(dec.store, ws, dec.dims, mode=0, keep_gpre=False, alone=True)
        call("arcvae_dec_row_lse", ptr(ws.logits), ptr(lse), B * dec.vocab_size, dec.vocab_size, float(temperature), stream_ptr())
        return ws.logits, lse, B

    def generate_map(self, z, conditions, max_length: int = 80, temperature: float = 1.0, min_length: int = 0,
                     early_stopping: bool = True):
        """Extension (absent in the reference): the MOST PROBABLE sequence per row under log_softmax(logits / T), exactly -- a
        Viterbi recursion over the dense table (include/arcvae_hip.h arcvae_dec_viterbi) -> (tokens [B, L] int32, scores [B]
        float32).  z is accepted and unused (Q2).  A sequence ends with its first end_token, not before step min_length, or runs
        to max_length without one; positions after the end hold pad_token; ties go to the earliest end, then the lowest tokens.
        early_stopping: L = the longest returned sequence; otherwise L = max_length.  Each score equals
        decoder.sequence_log_prob of its tokens bit for bit, and is never below generate_beam's best at any width."""
        import ctypes as C
        T = int(max_length)
        if T < 1 or not 0 <= int(min_length) <= T:
            raise ValueError("need max_length >= 1 and 0 <= min_length <= max_length")
        if not 0 <= self.pad_token <= 255:
            raise ValueError("exact decoding needs 0 <= pad_token <= 255")
        logits, lse, B = self._chain_table(conditions, T, temperature)
        V, dev = self.decoder.vocab_size, self.decoder.store.device
        nbytes = C.c_long(0)
        call("arcvae_dec_viterbi_ws_bytes", B, V, T, C.byref(nbytes))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        lengths = torch.empty(B, dtype=torch.int32, device=dev)
        call("arcvae_dec_viterbi", ptr(logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch), nbytes.value, B, V,
             T, int(min_length), self.end_token, self.pad_token, float(temperature), stream_ptr())
        if early_stopping:
            tokens = tokens[:, :int(lengths.max().item())].contiguous()
        return tokens, scores

    def generate_kbest(self, z, conditions, max_length: int = 80, num_best: int = 4, temperature: float = 1.0, min_length: int = 0,
                       early_stopping: bool = True):
        """Extension (absent in the reference): the num_best MOST PROBABLE sequences per row under log_softmax(logits / T), exactly
        -- a list-Viterbi recursion over the dense table (include/arcvae_hip.h arcvae_dec_kbest) -> (tokens [B, K, L] int32,
        scores [B, K] float32, descending).  z is accepted and unused (Q2).  Sequences, min_length and padding as in generate_map;
        the K sequences of a row are pairwise distinct, rank 0 is generate_map's, and no rank is below generate_beam's at
        beam_width = num_best.  A slot that no sequence fills (num_best above the number of admissible sequences) has score -inf
        and pad tokens.  early_stopping: L = the longest returned sequence (at least 1); otherwise L = max_length.  Each score
        equals decoder.sequence_log_prob of its tokens bit for bit; exp(scores).sum(1) is the probability mass the list covers."""
        import ctypes as C
        K, T = int(num_best), int(max_length)
        if not 1 <= K <= 32:
            raise ValueError("num_best must lie in [1, 32]")
        if T < 1 or not 0 <= int(min_length) <= T:
            raise ValueError("need max_length >= 1 and 0 <= min_length <= max_length")
        if not 0 <= self.pad_token <= 255:
            raise ValueError("exact decoding needs 0 <= pad_token <= 255")
        logits, lse, B = self._chain_table(conditions, T, temperature)
        V, dev = self.decoder.vocab_size, self.decoder.store.device
        nbytes = C.c_long(0)
        call("arcvae_dec_kbest_ws_bytes", B, V, K, T, C.byref(nbytes))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        tokens = torch.empty(B, K, T, dtype=torch.int32, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
        call("arcvae_dec_kbest", ptr(logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch), nbytes.value, B, V,
             K, T, int(min_length), self.end_token, self.pad_token, float(temperature), stream_ptr())
        if early_stopping:
            tokens = tokens[:, :, :max(int(lengths.max().item()), 1)].contiguous()
        return tokens, scores

    def token_marginals(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """Extension (absent in the reference): [B, max_length, V] float32, entry [b, t, v] = P(the token at step t is v and no
        end_token came before t) of what sample=True draws at this temperature -- the chain's forward recursion, exact up to fp32
        rounding (include/arcvae_hip.h arcvae_dec_chain_marginals).  Column end_token is the length distribution."""
        T = int(max_length)
        logits, lse, B = self._chain_table(conditions, T, temperature)
        V = self.decoder.vocab_size
        alive = torch.empty(B, T, V, dtype=torch.float32, device=self.decoder.store.device)
        call("arcvae_dec_chain_marginals", ptr(logits), ptr(lse), ptr(alive), B, V, T, self.end_token, float(temperature),
             stream_ptr())
        return alive

    def length_distribution(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """[B, max_length + 1] float32: entry t < max_length = P(length = t+1) (the end_token column of token_marginals), the
        last entry = P(no end_token within max_length), the mass a max_length cuts off."""
        alive = self.token_marginals(conditions, max_length, temperature)
        last = alive[:, -1, :]
        rest = last.sum(dim=1) - last[:, self.end_token]
        return torch.cat([alive[:, :, self.end_token], rest[:, None]], dim=1)
