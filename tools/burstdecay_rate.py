#!/usr/bin/env python3
"""Device time of the burst-decay map on 256 synthetic 480 000-sample IRs (10 s at 48 kHz) at the default settings (8
cycles, 24 points per octave, 20 Hz .. 20 kHz, 61 steps of half a period: 240 points, 41.1 M terms per channel with whole
windows), from the engine's events, median and min .. max of 7 after 2 warm-ups: the two calls together, ira_burst_table
alone, the terms summed (the terms inside the channels, counted on the host) and their rate, and the end-to-end
analyse_burst_decay_batch time (upload, peak and onset, the map's way back to the host and the host arithmetic included).
The yardstick: the SAME ms-axis hann map (151 steps of 2 ms) made by 151 calls of ira_fdw_response, one per step with the
centres p + delta_m -- the same number of terms, weight and phasor made anew for every term -- against ira_burst_table +
ira_burst_decay on that axis, the two routes alternating run by run; their sums are compared cell by cell first.
--one-call: one table call and one map call at the defaults after one warm-up, nothing else on the device -- the run a
kernel trace is taken from (per-launch times: profiles/README.md)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from audio_analysis_amd.analyse import burstdecay as D
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

B, N_SAMPLES, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N_SAMPLES, SR) for i in range(B)]
batch = eng.upload(host)

if "--one-call" in sys.argv:
    for _ in range(2):
        D.burst_decay_device(eng, batch, SR, D.BurstDecaySettings())
        eng.sync()
    sys.exit(0)


def events_of(call):
    eng.events = []
    res = call()
    ev = eng.collect_events()
    eng.events = None
    return res, ev


def total_ms(ev, prefix):
    return sum(float(np.sum(v)) for k, v in ev.items() if k.startswith(prefix))


def spread(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def terms_of(res):
    return float(sum(int(D.terms_inside(int(res.centre[c]), res.delta, res.half, int(res.length[c])).sum()) for c in range(B)))


def fdw_route(st, rho, half, delta, centre_dev):
    """The ms-axis map by one ira_fdw_response call per step; returns (nch, J, M, 2) device."""
    cols = [eng.fdw_response(batch.x, batch.off, batch.length, centre_dev + int(delta[0, m]), rho, half, st.window)[:, :, :2]
            for m in range(delta.shape[1])]
    return eng.torch.stack(cols, dim=2)


rows = []
# ---- the default map
st = D.BurstDecaySettings()
both, tab = [], []
for rep in range(WARM + REPS):
    res, ev = events_of(lambda: D.burst_decay_device(eng, batch, SR, st))
    if rep >= WARM:
        tab.append(total_ms(ev, "ira_burst_table"))
        both.append(tab[-1] + total_ms(ev, "ira_burst_decay"))
terms = terms_of(res)
names = [str(h) for h in range(B)]
D.analyse_burst_decay_batch(host, SR, names, st)
eng.sync()
t0 = time.perf_counter()
D.analyse_burst_decay_batch(host, SR, names, st)
e2e = time.perf_counter() - t0
both, tab = spread(both), spread(tab)
row = dict(what="default map", axis=st.axis, window=st.window, irs=B, samples=N_SAMPLES, points=int(res.half.size),
           steps=int(res.axis_values.size), terms=terms, table_and_map_ms=both, table_ms=tab,
           terms_per_ns=terms / ((both[0] - tab[0]) * 1e6), out_bytes=int(res.sums.nbytes), end_to_end_s=e2e)
rows.append(row)
print(f"default ({st.axis}, {st.window}): {row['points']} points x {row['steps']} steps, {terms / 1e9:.2f} G terms;  table + map "
      f"{both[0]:.3f} ms ({both[1]:.3f} .. {both[2]:.3f}), table alone {tab[0]:.3f} ms ({tab[1]:.3f} .. {tab[2]:.3f}), "
      f"{row['terms_per_ns']:.1f} terms/ns in the map;  end-to-end {e2e * 1e3:.0f} ms for {row['out_bytes'] / 1e6:.0f} MB of map",
      flush=True)

# ---- the yardstick: the ms-axis hann map, new route against one ira_fdw_response call per step
st = D.BurstDecaySettings(axis="ms")
f, rho, half, t, delta = D.burst_grid(st, SR)
centre_dev = eng.onset_index(batch, st.rel_energy)[1]
new = D.burst_decay_device(eng, batch, SR, st)
old = fdw_route(st, rho, half, delta, centre_dev).cpu().numpy()
scale = float(np.max(np.abs(old)))
gap = float(np.max(np.abs(new.sums - old)))
print(f"ms axis: largest |new - old| over the map {gap:.3e}, largest |S| {scale:.3e}", flush=True)
assert gap <= 1e-9 * scale, "the two routes disagree"
del old
new_ms, new_tab, old_ms = [], [], []
for rep in range(WARM + REPS):
    _, ev = events_of(lambda: D.burst_decay_device(eng, batch, SR, st))
    _, ev_old = events_of(lambda: fdw_route(st, rho, half, delta, centre_dev))
    if rep >= WARM:
        new_tab.append(total_ms(ev, "ira_burst_table"))
        new_ms.append(new_tab[-1] + total_ms(ev, "ira_burst_decay"))
        old_ms.append(total_ms(ev_old, "ira_fdw_response"))
terms = terms_of(new)
new_ms, new_tab, old_ms = spread(new_ms), spread(new_tab), spread(old_ms)
row = dict(what="yardstick", axis="ms", window="hann", irs=B, samples=N_SAMPLES, points=int(half.size), steps=int(t.size),
           terms=terms, table_and_map_ms=new_ms, table_ms=new_tab, fdw_calls=int(t.size), fdw_route_ms=old_ms,
           ratio=old_ms[0] / new_ms[0], terms_per_ns=terms / ((new_ms[0] - new_tab[0]) * 1e6),
           fdw_terms_per_ns=terms / (old_ms[0] * 1e6), largest_gap=gap, largest_value=scale)
rows.append(row)
print(f"yardstick (ms, hann): {row['points']} points x {row['steps']} steps, {terms / 1e9:.2f} G terms;  table + map {new_ms[0]:.3f} "
      f"ms ({new_ms[1]:.3f} .. {new_ms[2]:.3f}), {row['terms_per_ns']:.1f} terms/ns in the map;  {row['fdw_calls']} ira_fdw_response "
      f"calls {old_ms[0]:.3f} ms ({old_ms[1]:.3f} .. {old_ms[2]:.3f}), {row['fdw_terms_per_ns']:.1f} terms/ns;  ratio "
      f"{row['ratio']:.2f}", flush=True)
print(json.dumps(rows))
