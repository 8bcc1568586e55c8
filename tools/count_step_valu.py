#!/usr/bin/env python3
"""Count the VALU instructions of the step loop of a systolic DP kernel (k_scan of scan.hip, k_align_fwd of align.hip,
k_align_band of band.hip with --rows 24; the step body they share is csrc/systolic.h) in gfx950 assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only -S -o scan.s scan.hip
    tools/count_step_valu.py scan.s _ZN5fasim6k_scanILi22ELb0ELb1ELb0EEEvNS_8ScanArgsE [--rows 22] [--blocks]

The step loop is the innermost loop (backward branch) that holds at least `rows` v_perm_b32 (one per DP row and step).  Its
basic blocks are split into the common path and the rare ones: a block is rare when it holds an instruction that only the
hazard branch and the bookkeeping at block ends use (v_pk_min_u16, v_cvt_u16_f16, v_or_b32 in place,
v_pk_add_f16 in place, global stores of the snapshots / block maxima / lane maxima) and holds no row work (v_perm_b32).
The loop holds both variants of the hand-over from virtual lane v - 1 (first query tile: zeros enter through DPP bound_ctrl;
later tiles: the previous tile's bottom row enters through v_readlane); a launch runs one of them, so the count is given for
each.  Printed: VALU instructions of the common path per step (the loop may hold several steps: v_perm_b32 / rows) and the
mnemonic histogram.  --blocks lists every block of the loop with its verdict.
"""
import argparse
import collections
import re
import sys


def function_lines(path, symbol):
    out, on = [], False
    for line in open(path):
        if not on:
            if line.startswith(symbol + ":"):
                on = True
            continue
        if line.startswith(".Lfunc_end"):
            break
        out.append(line.rstrip("\n"))
    if not out:
        sys.exit(f"{symbol}: not found in {path}")
    return out


def parse(lines):
    """-> list of ('label', name) / ('ins', mnemonic, operands)"""
    items = []
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            items.append(("label", m.group(1)))
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)\s*(.*?)\s*(;.*)?$", ln)
        if m and not ln.lstrip().startswith((".", ";")):
            items.append(("ins", m.group(1), m.group(2)))
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--rows", type=int, default=22)
    ap.add_argument("--blocks", action="store_true")
    args = ap.parse_args()
    items = parse(function_lines(args.asm, args.symbol))
    pos = {it[1]: k for k, it in enumerate(items) if it[0] == "label"}
    spans = []
    for k, it in enumerate(items):
        if it[0] == "ins" and it[1].startswith(("s_cbranch", "s_branch")):
            t = it[2].split()[0] if it[2] else ""
            if t in pos and pos[t] < k:
                nperm = sum(1 for x in items[pos[t]:k] if x[0] == "ins" and x[1] == "v_perm_b32")
                if nperm >= args.rows:
                    spans.append((k - pos[t], pos[t], k, nperm))
    if not spans:
        sys.exit("no loop with enough v_perm_b32 found")
    _, a, b, nperm = min(spans)
    steps = nperm // args.rows
    # basic blocks of the loop
    blocks, cur = [], {"label": items[a][1], "ins": []}
    for it in items[a + 1:b + 1]:
        if it[0] == "label":
            blocks.append(cur)
            cur = {"label": it[1], "ins": []}
        else:
            cur["ins"].append(it)
            if it[1].startswith(("s_cbranch", "s_branch")):
                blocks.append(cur)
                cur = {"label": None, "ins": []}
    if cur["ins"] or cur["label"]:
        blocks.append(cur)

    def rare_ins(it):
        mn, ops = it[1], [o.strip() for o in it[2].split(",")]
        if mn in ("v_pk_min_u16", "v_cvt_u16_f16_e32", "v_cvt_u16_f16_sdwa", "v_cvt_u16_f16"):
            return True
        if mn in ("v_or_b32_e32", "v_or_b32") and len(ops) == 3 and ops[0] == ops[1]:
            return True
        if mn == "v_pk_add_f16" and len(ops) == 3 and ops[0] == ops[1]:
            return True
        return mn.startswith("global_store")

    for blk in blocks:
        # (a block with row work is on the common path whatever else it holds)
        blk["rare"] = any(rare_ins(it) for it in blk["ins"]) and not any(it[1] == "v_perm_b32" for it in blk["ins"])
        blk["valu"] = sum(1 for it in blk["ins"] if it[1].startswith("v_"))
        dpp = [it for it in blk["ins"] if it[1] == "v_mov_b32_dpp"]
        blk["tile"] = None
        if dpp and not blk["rare"] and not any(it[1] == "v_perm_b32" for it in blk["ins"]):
            if any("bound_ctrl" in it[2] for it in dpp):
                blk["tile"] = "first"
            elif sum(1 for it in blk["ins"] if it[1] == "v_readlane_b32") >= 2:
                blk["tile"] = "later"
    hist = collections.Counter()
    common = total = 0
    only = {"first": 0, "later": 0}
    for blk in blocks:
        total += blk["valu"]
        if not blk["rare"]:
            common += blk["valu"]
            if blk["tile"]:
                only[blk["tile"]] += blk["valu"]
            hist.update(it[1] for it in blk["ins"] if it[1].startswith("v_"))
        if args.blocks:
            print(f"  block {blk['label'] or '(fallthrough)':14s} {'rare  ' if blk['rare'] else (blk['tile'] + ' ' if blk['tile'] else 'common')} VALU {blk['valu']:4d}  instructions {len(blk['ins']):4d}")
    print(f"{args.symbol}: step loop of {steps} step(s), VALU on the common path per step: "
          f"{(common - only['later']) / steps:.1f} (first tile), {(common - only['first']) / steps:.1f} (later tiles); "
          f"{total / steps:.1f} with the rare blocks and both hand-over variants")
    print("  " + ", ".join(f"{n} {m}" for m, n in hist.most_common(14)))


if __name__ == "__main__":
    main()
