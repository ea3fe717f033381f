"""The quantised modes of the block linears at model level on the MI355X, one routine per check over the rows of tests/quant_modes.py:
one real-shape block against the mode's host oracle (tests/quant_ref.py), the 30-layer steady state and config 2 free-running against
the reference's bf16 goldens (and near or apart from the neighbouring mode's run), and the mode beside MX self-attention on the toy
model.  Every full-depth run and every host oracle of a block is computed once per module and shared.  The op-level pins of each
format (lane maps, quantiser bytes, epilogues, random data, outliers) are in tests/test_ops_gpu.py, test_mx_gpu.py, test_fp8_gpu.py,
test_mx6_gpu.py, test_mx4_gpu.py and test_mx4a4_gpu.py."""
import pytest
import torch

import mx_attn_ref as MA
from conftest import load_golden
from longlive_amd import synth
from model_runs import RealBlock, config2_run, have, real30, steady_flow, toy, toy_caches  # noqa: F401  (real30: module fixture)
from oracle import ref_model as RM
from quant_modes import MODES
from quant_ref import make_ref
from util import cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _name(mode):
    return "bf16" if mode is None else mode


class _Runs:
    """Each mode's runs on first request, kept on the host: a mode that serves as another's neighbour is not run again, and any
    test selected alone computes what it needs."""

    def __init__(self):
        self._memo = {}

    def _once(self, key, compute):
        if key not in self._memo:
            self._memo[key] = compute()
        return self._memo[key]

    @staticmethod
    def _in_mode(real30, mode, run):
        real30[1].model.set_quant(mode)
        try:
            return run()
        finally:
            real30[1].model.set_quant(None)

    def steady(self, real30, mode):
        """The flow of the 30-layer steady-state forward."""
        return self._once(("steady", mode), lambda: self._in_mode(real30, mode, lambda: steady_flow(real30)))

    def config2(self, real30, mode):
        """The 21 latent frames of config 2, free-running."""
        return self._once(("config2", mode),
                          lambda: self._in_mode(real30, mode, lambda: config2_run(real30, teacher=False, check=False)[2].cpu()))

    def block(self, seed):
        return self._once(("block", seed), lambda: RealBlock(seed))

    def block_oracle(self, seed, mode):
        """The mode's host oracle on the block of `seed`: (output, 64 sampled cache slots of k and of v, end indices)."""
        def compute():
            blk = self.block(seed)
            y, kvr, planr = blk.oracle(lambda cfg, sd, **kw: make_ref(mode, cfg, sd, **kw))
            return y, kvr["k"][0, blk.slots], kvr["v"][0, blk.slots], (planr["G_new"], planr["E_new"])
        return self._once(("oracle", seed, mode), compute)


@pytest.fixture(scope="module")
def runs():
    return _Runs()


@pytest.mark.parametrize("mode", list(MODES))
def test_block_vs_oracle(runs, mode):
    """One real-shape block in steady state (Lk = 18720, roll + insert) against the mode's oracle: the arithmetic pinned to its
    DEFINITION, not just to "close to bf16".  The bound must exclude the row's other oracles (the own oracle's distance to each is
    asserted above it), or the output must sit closer to its own oracle than to them.  int8's bound cannot be much tighter than the
    bf16 block test's: a 1-ulp bf16 difference in a row's LARGEST activation (GPU vs CPU accumulation order) changes that token's
    scale, and with it the int8 codes of a few per cent of the row -- two valid quantisations whose rounding noise is partly
    independent; what IS exact is checked at op level."""
    row = MODES[mode]
    blk = runs.block(row.seed)
    if row.block_packs_of is not None:
        try:
            packs = {kk: vv.clone() for kk, vv in blk.m.set_quant(row.block_packs_of)._pack()[0].items() if kk[:2] in ("q_", "s_")}
            mine = blk.m.set_quant(mode)._pack()[0]
            assert len(packs) == 12 and all(torch.equal(mine[kk], vv) for kk, vv in packs.items())
        finally:
            blk.m.set_quant(None)
    got, kv = blk.run(mode)
    got_bf = blk.run(None)[0]
    own, k_slots, v_slots, idx = runs.block_oracle(row.seed, mode)
    others = {o: runs.block_oracle(row.seed, o)[0] for o in dict.fromkeys(row.block_exclude + row.block_closer_than)}
    r, c = rel_l2(got, own), cosine(got, own)
    to_other = {o: rel_l2(got, y) for o, y in others.items()}
    own_to_other = {o: rel_l2(own, y) for o, y in others.items()}
    print(f"{mode} block: vs {mode} oracle relL2 {r:.2e} (cos {c:.6f}); "
          + "".join(f"vs {_name(o)} oracle {to_other[o]:.2e}, " for o in others)
          + "".join(f"{mode} oracle vs {_name(o)} oracle {own_to_other[o]:.2e}, " for o in others)
          + (f"block update size {rel_l2(blk.x0.cpu(), others[None]):.2e}, " if None in others else "")
          + f"the same block, {mode} vs bf16 on the GPU: {rel_l2(got, got_bf):.2e}; bound {row.block.rel:.2e}")
    for o in row.block_exclude:
        assert own_to_other[o] > row.block.rel, (o, own_to_other[o], row.block.rel)
    for o in row.block_closer_than:
        assert r < to_other[o], (o, r, to_other[o])
    assert row.block.holds(r, c), (r, c)
    assert (kv["global_end_index"], kv["local_end_index"]) == idx
    rk, rv = rel_l2(kv["k"].cpu()[0, blk.slots], k_slots), rel_l2(kv["v"].cpu()[0, blk.slots], v_slots)
    print(f"{mode} block: cache slots vs {mode} oracle k {rk:.2e} v {rv:.2e}")
    assert rk < 5e-3 and rv < 5e-3, (rk, rv)


@pytest.mark.skipif(not have("real_fwd.pt"), reason="golden missing")
@pytest.mark.parametrize("mode", list(MODES))
def test_steady_state_vs_reference(runs, real30, mode):
    """30 layers in the regime the mode runs in (roll + insert, Lk = 18720) against the reference's bf16 CPU golden
    (`real_fwd.pt:flow_steady`), and against the neighbouring mode's run: within the row's band of it, or apart from it (so the
    mode is on)."""
    row = MODES[mode]
    rec = load_golden("real_fwd.pt")
    own, nb = runs.steady(real30, mode), runs.steady(real30, row.neighbour)
    r, c = rel_l2(own, rec["flow_steady"]), cosine(own, rec["flow_steady"])
    r_nb, c_nb = rel_l2(own, nb), cosine(own, nb)
    print(f"{mode} steady: vs reference bf16 {r:.2e} (cos {c:.6f}); vs the {_name(row.neighbour)} run {r_nb:.2e} (cos {c_nb:.6f}); "
          f"the {_name(row.neighbour)} run vs reference {rel_l2(nb, rec['flow_steady']):.2e}")
    assert row.steady.holds(r, c), (r, c)
    if row.near is not None:
        assert row.near.holds(r_nb, c_nb), (r_nb, c_nb)
    if row.apart is not None:
        assert r_nb > row.apart, r_nb


@pytest.mark.skipif(not have("config2_pipe.pt"), reason="golden missing")
@pytest.mark.parametrize("mode", list(MODES))
def test_config2_free_running_vs_reference_bf16(runs, real30, mode):
    """The mode's arithmetic THROUGH THE AR LOOP: the 21-frame run of config 2, free-running (its own x0 re-noised, its own caches
    through the roll), against the reference's bf16 latents.  The reference ships none of these modes, so this is a distance, not a
    parity: per block within the row's band, apart from the neighbouring mode's run in every block where the row says so, and it must
    not GROW along the stream: the last block within 1.25x of the first."""
    row = MODES[mode]
    want = load_golden("config2_pipe.pt")["latents"]
    own = runs.config2(real30, mode)
    nb = runs.config2(real30, row.neighbour) if row.apart is not None else None
    rs = []
    for blk in range(7):
        sl = slice(3 * blk, 3 * blk + 3)
        r, c = rel_l2(own[:, sl], want[:, sl]), cosine(own[:, sl], want[:, sl])
        rs.append(r)
        r_nb = None if nb is None else rel_l2(own[:, sl], nb[:, sl])
        print(f"config 2 {mode} free-running: block {blk} latents vs reference bf16: relL2 {r:.2e} cos {c:.6f}"
              + ("" if nb is None else f"; vs {row.neighbour} run {r_nb:.2e}"))
        assert row.config2.holds(r, c), (blk, r, c)
        if nb is not None:
            assert r_nb > row.apart, (blk, r_nb)
    assert (rs[-1] <= 1.25 * rs[0]) if row.growth_inclusive else (rs[-1] < 1.25 * rs[0]), rs


@pytest.mark.parametrize("mode", [m for m, row in MODES.items() if row.toy is not None])
def test_with_mx_attention_toy_vs_oracle(mode):
    """set_quant(mode) + set_attn_quant("mxfp8") on the toy model over fill, roll and the next frames, against a host model with the
    mode's linears and tests/mx_attn_ref.py's attention; it must sit closer to that oracle than to the one with the row's other
    linears."""
    check = MODES[mode].toy
    cfg, sd, gen, S = toy("mxfp8", mode)
    fs = cfg.frame_seqlen
    kv, ca = toy_caches(cfg, S, DEV)
    noise = synth.synth_noise(cfg, 5, seed=5)
    prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9)
    oracles = {}
    for lin in (mode, check.other):
        om = MA.MXAttnRefModel(RM.RefConfig.from_cfg(cfg), sd, frame_seqlen_for_max_attn=fs, linears=lin)
        oracles[lin] = (RM.RefGenerator(om, 5.0), RM.new_kv_cache(1, S, cfg.num_layers, cfg.num_heads, 128),
                        RM.new_crossattn_cache(1, cfg.text_len, cfg.num_layers, cfg.num_heads, 128))
    worst = dict.fromkeys(oracles, 0.0)
    try:
        for f in range(5):                       # fill, then rolls
            x = noise[:, f:f + 1]
            t = torch.full((1, 1), 937.5)
            _, x0 = gen(x.to(DEV), {"prompt_embeds": prompt.to(DEV)}, t.to(DEV), kv_cache=kv, crossattn_cache=ca, current_start=f * fs)
            for lin, (og, okv, oca) in oracles.items():
                _, r0 = og(x, prompt, t, okv, oca, f * fs)
                worst[lin] = max(worst[lin], rel_l2(x0.cpu(), r0))
    finally:
        gen.model.set_quant(None).set_attn_quant(None)
    print(f"{mode} + MX attention, toy: worst x0 rel-L2 vs the {mode} + MX-attention oracle {worst[mode]:.2e}, vs the "
          f"{_name(check.other)}-linear one {worst[check.other]:.2e}; bound {check.bound:.2e}")
    assert worst[mode] < check.bound, worst
    assert worst[mode] < worst[check.other], worst
