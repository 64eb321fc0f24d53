"""RealtimeAgentBatch -- N RealtimeAgents over one set of LM weights, one tick at a time.

A server that keeps many duplex sessions on a card gives every session its own RealtimeAgent (own sequence, codec windows, sampler,
statistics) over weight-sharing LM handles (RealtimeAgentResources.clone_for_self_play) and ONE codec handle, and calls
process_audio(chunks) once per tick.  The sessions whose frame can run as one replay (RealtimeAgent._replay_plan: both codec windows
full, audio mode, nothing forced, no trim between two steps) are grouped by call shape, and every group of at least `min_batch` takes ONE
LlamaBatch.duplex_frame (rca_duplex_batch_frame); every other session with a chunk runs its own process_audio unchanged.

A batch frame is in the tile arithmetic class (LlamaBatch): a session inside the batch samples other tokens than the same session
alone -- equally valid ones; with use_duplex_batch_graph=False the ready group runs the same LM arithmetic through the separate calls
(tokenize_audio, one LlamaBatch.frame(members=...), detokenize_output_chunk), so the two can be compared, as use_duplex_graph does for
one session.

batch_speaker_step=True (off by default) also batches the agents' speculative <|end_audio|> step: the fused members of a tick commit
with the step deferred, and those that owe it (z-score of P(<|end_audio|>) >= 0) take ONE LlamaBatch.step_probe
(rca_lm_batch_step_sel) when there are at least min_batch of them, else their own single steps.  That moves the two speaker
probabilities and the step's throw-away draw into the tile arithmetic class too.

batch_shadow_tiles=True (off by default) feeds the shadow-cache tiles that fall due in a tick (kv_shadow.py: one 128-token tile per
session every ~16 ticks) to the sessions' twins in ONE LlamaBatchEval.eval_async (rca_lm_batch_eval) instead of one eval_async per
session, each a pass over all weights.  A twin ends with the bits of its own eval_async, so tokens, PCM and caches are those of the
flag off.  LMs without the call (llama.cpp objects, test fakes, models off the 128-token tiles) keep the per-session advance.

batch_shift_trims=True (off by default) is for sessions in kv_trim_mode="shift": the context shifts that fall due while a tick is
planned (sessions admitted together reach max_context_secs on the same tick) are recorded instead of issued, and ONE kv_remove_many
(rca_lm_kv_remove_many) runs them before the tick's first LM call when there are at least two; a single one takes kv_remove.  Every
cache ends with the bits of its own kv_remove, so tokens, PCM and caches are those of the flag off.  A trim that falls between two
steps of a frame stays with its session, and so do LM objects without kv_remove_many.
Not thread-safe: one caller per tick."""
from typing import List, Optional, Sequence, Tuple

import numpy as np


class RealtimeAgentBatch:
    def __init__(self, agents: Sequence, min_batch: int = 4, use_duplex_batch_graph: bool = True, batch_speaker_step: bool = False,
                 batch_shadow_tiles: bool = False, batch_shift_trims: bool = False):
        self.agents = list(agents)
        # where one batch call starts to win over as many single calls: 4, the smallest size measured, for the frame (profiles/r16:
        # 11.0 against 13.8 ms) and for the speaker step (profiles/r18: 2.64 against 3.29 ms; three single steps are 2.5 ms)
        self.min_batch = max(1, int(min_batch))
        self.use_duplex_batch_graph = bool(use_duplex_batch_graph)
        self.fused_ticks = 0       # ticks in which at least one group took the batch call
        self.fused_frames = 0      # agent frames that went through it
        self.batch_speaker_step = bool(batch_speaker_step)
        self.fused_speaker_calls = 0   # batch step_probe calls for the speculative <|end_audio|> step
        self.fused_speaker_steps = 0   # agents' speculative steps that went through them
        self.batch_shadow_tiles = bool(batch_shadow_tiles)
        self.fused_shadow_calls = 0    # LlamaBatchEval calls that fed the shadow tiles of several sessions
        self.fused_shadow_tiles = 0    # tiles that went through them
        self.batch_shift_trims = bool(batch_shift_trims)
        self.fused_shift_calls = 0     # kv_remove_many calls that ran the context shifts of several sessions
        self.fused_shift_trims = 0     # trims that went through them
        self._batch = None
        self._shadow_pool = None
        if len(self.agents) < 2:
            raise ValueError("a RealtimeAgentBatch drives at least two agents")
        llms = [a.resources.llm for a in self.agents]
        if len({id(m) for m in llms}) != len(llms):
            raise ValueError("every agent needs an LM handle of its own (RealtimeAgentResources.clone_for_self_play)")
        first = self.agents[0]
        for i, a in enumerate(self.agents[1:], 1):
            for what in ("_code_token_base", "end_header_token_id", "end_audio_token_id"):
                if getattr(a, what) != getattr(first, what):
                    raise ValueError(f"agent {i} has another {what.lstrip('_')} than agent 0 ({getattr(a, what)} / {getattr(first, what)})")
            if self._codec(a) is not self._codec(first):
                raise ValueError(f"agent {i} uses another codec handle than agent 0")
        if all(hasattr(m, "duplex_frame") and hasattr(m, "_h") for m in llms) and self._codec(first) is not None:
            from . import _native as N
            from .llm import LlamaBatch
            try:
                self._batch = LlamaBatch(llms)
            except N.RcaError as e:       # other weights, another device, a model off the tile route
                raise ValueError(f"the agents' LMs cannot form one batch: {e}") from e
        if self.batch_shadow_tiles and all(hasattr(m, "_h") for m in llms):
            from .llm import LlamaBatchEval
            if all(LlamaBatchEval.supported(m) for m in llms):
                self._shadow_pool = LlamaBatchEval(llms[0])

    @staticmethod
    def _codec(agent):
        return getattr(agent.resources.audio_tokenizer.codec_model, "hip", None)

    # ------------------------------------------------------------------ who runs how
    def _partition(self, plans: Sequence[Optional[dict]]) -> Tuple[List[List[int]], List[int]]:
        """plans[i]: agent i's plan, or None (no chunk, or not ready).  Returns (groups, rest): the ready agents grouped by call shape,
        groups of at least min_batch only, each in agent order; and the other ready agents, which run on their own."""
        by_shape = {}
        for i, p in enumerate(plans):
            if p is not None:
                shape = (len(p["window"]) if np.ndim(p["window"]) == 1 else np.shape(p["window"])[-1], len(p["code_ctx"]), p["n_codes"], p["n_samples"])
                by_shape.setdefault(shape, []).append(i)
        groups = [g for g in by_shape.values() if len(g) >= self.min_batch]
        rest = sorted(i for g in by_shape.values() if len(g) < self.min_batch for i in g)
        return groups, rest

    def process_audio(self, chunks: Sequence[Optional[np.ndarray]]) -> list:
        """One chunk or None per agent in, one RealtimeAgent.process_audio result or None per agent out."""
        if len(chunks) != len(self.agents):
            raise ValueError(f"{len(chunks)} chunks for {len(self.agents)} agents")
        outs = [None] * len(self.agents)
        live = [i for i, c in enumerate(chunks) if c is not None]
        for i in live:
            self.agents[i]._settle_shadow()
        plans = [None] * len(self.agents)
        if self._batch is not None:
            sink = [] if self.batch_shift_trims else None
            for i in live:
                a = self.agents[i]
                a._shift_sink = sink                # the trim check of the plan records its context shift instead of issuing it
                try:
                    plans[i] = a._replay_plan(chunks[i])
                finally:
                    a._shift_sink = None
            if sink:
                self._flush_shift_trims(sink)       # before any LM call of the tick
        groups, _ = self._partition(plans)
        fused = {i for g in groups for i in g}
        for g in groups:
            self._run_group(g, chunks, plans, outs)
        for i in live:
            if i not in fused:
                outs[i] = self.agents[i].process_audio(chunks[i])     # settles and advances its own shadow cache
        if self.batch_speaker_step:
            self._run_speaker_steps(sorted(fused))
        self._advance_shadows(sorted(fused))
        if groups:
            self.fused_ticks += 1
            self.fused_frames += len(fused)
        return outs

    def _flush_shift_trims(self, due: list) -> None:
        """The context shifts (llm, p0, p1) the planning loop recorded: one kv_remove_many for two or more of them when every LM object
        offers it, else every session's own kv_remove, in the order they fell due."""
        llms = [m for m, _, _ in due]
        if len(due) >= 2 and all(hasattr(m, "kv_remove_many") for m in llms) and len({id(m) for m in llms}) == len(llms):
            llms[0].kv_remove_many(llms, [(p0, p1) for _, p0, p1 in due])
            self.fused_shift_calls += 1
            self.fused_shift_trims += len(due)
            return
        for m, p0, p1 in due:
            m.kv_remove(p0, p1)

    def _advance_shadows(self, fused: List[int]) -> None:
        """The end of a tick for the fused members: every shadow cache is planned as RealtimeAgent._advance_shadow plans it; the tiles
        that are due go to their twins in one LlamaBatchEval call when there is a pool and more than one of them, else through the
        session's own advance."""
        A = self.agents
        if self._shadow_pool is None or not self.batch_shadow_tiles:
            for i in fused:
                A[i]._advance_shadow()
            return
        due = []
        for i in fused:
            sh = A[i]._plan_shadow()
            tile = sh.next_tile(A[i].input_ids) if sh is not None else None
            if tile is not None:
                due.append((sh, tile, i))
        if len(due) == 1:
            due[0][0].advance(A[due[0][2]].input_ids)
        elif due:
            self._shadow_pool.eval_async([sh.twin for sh, _, _ in due], [tile for _, tile, _ in due], want_logits=False)
            for sh, tile, _ in due:
                sh.commit_tile(tile)
            self.fused_shadow_calls += 1
            self.fused_shadow_tiles += len(due)

    def _run_speaker_steps(self, fused: List[int]) -> None:
        """The speculative <|end_audio|> steps the fused members of this tick deferred (across groups): one batch step_probe for at
        least min_batch of them, rolled back by one position per member; fewer take their own step."""
        A = self.agents
        owed = [i for i in fused if A[i].speaker_step_owed]
        for i in owed:
            A[i].speaker_step_owed = False
        if len(owed) < self.min_batch:
            for i in owed:
                A[i].prob_event_speaker_token_id = A[i].get_probable_event_speaker()
            return
        _, probs = self._batch.step_probe(owed, [[A[i].end_audio_token_id] for i in owed],
                                          [[A[i].agent_speaker_token_id, A[i].user_speaker_token_id] for i in owed])
        for (pa, pu), i in zip(probs, owed):
            A[i].resources.llm.n_tokens -= 1
            A[i]._set_probable_event_speaker(pa, pu)
        self.fused_speaker_calls += 1
        self.fused_speaker_steps += len(owed)

    def _run_group(self, sel: List[int], chunks, plans, outs) -> None:
        A = self.agents
        defer = self.batch_speaker_step
        first, p0 = A[sel[0]], plans[sel[0]]
        pairs = [A[i].input_ids[-2:] for i in sel]
        probes = [first.end_audio_token_id] * len(sel)
        if self.use_duplex_batch_graph:
            res = self._batch.duplex_frame(self._codec(first), sel, np.stack([np.reshape(plans[i]["window"], -1) for i in sel]),
                                           np.stack([plans[i]["code_ctx"] for i in sel]), p0["n_codes"], p0["n_samples"], first._code_token_base,
                                           first.end_header_token_id, probes, pairs)
            for k, i in enumerate(sel):
                a = A[i]
                with a.profilers.total_profiler:
                    out = a._replay_commit(chunks[i], plans[i], lambda r=res[k]: r, defer_speaker=defer)
                outs[i] = out if a.self_play_mode else out[0]
            return
        # the unfused path: the separate codec calls around ONE selection frame
        user_ids = []
        for i in sel:
            a, r = A[i], A[i].resources
            with a.profilers.audio_tokenize_profiler:
                s = r.audio_tokenizer.tokenize_audio(chunks[i])
            with a.profilers.tokenize_profiler:
                user_ids.append(r.tokenizer.encode(s, add_special_tokens=False))
        toks, probs = self._batch.frame(pairs, user_ids, first.end_header_token_id, probe_ids=probes, members=sel)
        for k, i in enumerate(sel):
            a = A[i]
            with a.profilers.total_profiler:
                with a.profilers.lm_profiler:
                    a.frame_graph_active = True
                    out_ids = a.process_audio_input_ids(user_ids[k], pre=toks[k])
                out_chunk = a.detokenize_output_chunk(out_ids)
                a.audio_history_ch2.append(chunks[i])
                a.measure_event_prob(None if np.isnan(probs[k]) else float(probs[k]), defer_speaker=defer)
                a.update_inactivity_timers()
            outs[i] = (out_chunk, out_ids) if a.self_play_mode else out_chunk

    def close(self) -> None:
        """the batch and the shadow pool first, then the agents' LM handles (shadow twins included)"""
        if self._shadow_pool is not None:
            self._shadow_pool.close()
            self._shadow_pool = None
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        for a in self.agents:
            sh = getattr(a, "_kv_shadow", None)
            if sh is not None and hasattr(sh.twin, "close"):
                sh.twin.close()
            if hasattr(a.resources.llm, "close"):
                a.resources.llm.close()
