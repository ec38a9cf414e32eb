#!/usr/bin/env python3
"""Check the generated gfx950 code of the decode kernels' prologues: the order of scalar loads, waits, barriers and
the first vector loads of every instance a batch-1 / batch-2 bf16 decode step dispatches.  Runs on the CPU.

    python tools/decode_prologue_isa.py                 # compiles csrc/kernels.hip (~3 minutes), checks, prints
    python tools/decode_prologue_isa.py --asm FILE.s    # checks an assembly file made earlier
    python tools/decode_prologue_isa.py --keep FILE.s   # keeps the assembly it compiled
    python tools/decode_prologue_isa.py --strict         # a second kernel-argument wait before the stream fails too

What fails an instance (exit status 1):
  * a scalar load through a pointer that was itself loaded (an SGPR pair that an earlier s_load wrote, or that
    was computed from one), anywhere in the prologue: the wave waits for it before anything behind it issues;
  * rows GEMV instances with the LayerNorm or embedding prologue: the first vmcnt wait behind the weight issue
    retires a weight load (the prologue would then start after the first weight chunk landed, not beside it;
    the merge prologue's and the head screen's loads sit in alternative branches, which a linear scan miscounts);
  * GEMV instances: anything but the kernel-argument wait between kernel entry and the first weight load: no
    vmcnt wait that retires a load, no barrier, no third s_waitcnt with scalar loads pending.  A second one (a
    second group of argument loads, hits in the scalar cache) is reported and fails only with --strict;
  * attention instances: a wait that retires a K/V load of the first chunk before q is staged (the first
    s_barrier), i.e. vmcnt(n) with n below the chunk's loads in flight; any vector or scalar load issued between
    that barrier and the first use of the chunk.

The scan is linear in text order (a branch's fall-through side); the listing it prints is what it judged.
The instance list is rows_plan / gemv_rows_launch / launch_attention / head_screen_launch of kernels.hip restated
below for the four BLOOM sizes; an instance the list names that the assembly lacks is an error.
head_rescore_kernel is listed without a verdict: its count[] / list[] reads are data dependencies of the
candidate tiles, loaded pointers by design.  gemv_head_screen_kernel (one launch per step) reads its arguments in
several groups, with the 64-bit tile-range divisions between them: the count is printed, not judged.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"bloom-560m": (1024, 16), "bloom-1b1": (1536, 16), "bloom-3b": (2560, 32), "bloom-7b1": (4096, 32)}
X_PLAIN, X_LN, X_PARTS, X_EMB = 0, 1, 2, 3
XM_NAME = {X_PLAIN: "plain", X_LN: "LN", X_PARTS: "parts", X_EMB: "emb"}


# ---- kernels.hip restated: tiles_take, rows_geometry, rows_plan, gemv_rows_launch ----
def tiles_take(M, K):
    return M >= 3 or (M == 2 and K >= 2560)


def rows_geometry(N, K, M, r_default):
    if M > 2:
        return r_default, 4
    rows_cu = (N + 255) // 256
    r = 2 if K <= 2048 else 1
    while (rows_cu + r - 1) // r > 16 and r < 4:
        r *= 2
    if (rows_cu + r - 1) // r < 4:
        r = 1
    return r, max(4, min(16, (rows_cu + r - 1) // r))


def rows_plan(XM, M, N, K):
    LN = XM in (X_LN, X_EMB)
    R0 = (2 if K <= 2048 else 1) if not LN else (4 if N >= 12288 else (2 if N >= 2048 else 1))
    R, waves = rows_geometry(N, K, M, R0)
    cpr = K // 512
    if K % 512:
        u = 4
    elif cpr <= 3 or cpr in (5, 8, 12):
        u = cpr
    else:
        u = 12 if cpr % 12 == 0 else (8 if cpr % 8 == 0 else (5 if cpr % 5 == 0 else 4))
    if waves > 4:
        cap = (12 if XM == X_PLAIN else 8) // (1 if M == 1 else 2)
        while R * u > cap:
            u = u // 2 if u % 2 == 0 else (4 if u > 4 else u - 1)
    if u not in (1, 2, 3, 5, 8, 12):
        u = 4
    return R, waves, u


def rows_instance(XM, M, N, K):
    """-> mangled-name prefix of the rows GEMV instance, or None where the tile GEMV takes the shape."""
    if XM in (X_PLAIN, X_LN) and tiles_take(M, K) and K % 64 == 0:
        return None
    R, waves, U = rows_plan(XM, M, N, K)
    LB = 256 if waves <= 4 else 1024
    return "_Z16gemv_rows_kernelILi%dELi%dELi%dELi%dELi0ELi%dEE" % (R, M, U, XM, LB)


def decode_instances():
    """(label, mangled prefix, kind) of every instance; kind: gemv / attn / screen / rescore."""
    out = {}

    def add(label, name, kind):
        if name is not None:
            out.setdefault((name, kind), []).append(label)

    for model, (h, nh) in MODELS.items():
        for M in (1, 2):
            tag = "%s B=%d" % (model, M)
            add(tag + " QKV", rows_instance(X_LN, M, 3 * h, h), "gemv")
            add(tag + " QKV(emb)", rows_instance(X_EMB, M, 3 * h, h), "gemv")
            add(tag + " fc1", rows_instance(X_LN, M, 4 * h, h), "gemv")
            add(tag + " fc2", rows_instance(X_PLAIN, M, h, 4 * h), "gemv")
            add(tag + " dense", rows_instance(X_PLAIN, M, h, h), "gemv")
            add(tag + " dense(parts)", rows_instance(X_PARTS, M, h, h), "gemv")
            # the exact head (EPI_ARGMAX): one 16-column tile per 4-wave block
            add(tag + " head", "_Z16gemv_rows_kernelILi4ELi%dELi%dELi1ELi0ELi256EE" % (M, 4 if h <= 2048 else 2), "gemv")
            # the greedy head's screen and re-score (head_screen_launch, launch_head_pick)
            cpr = (h + 511) // 512
            if cpr == 1:
                uu, rr = 1, 4
            elif cpr == 2:
                uu, rr = 2, 4
            elif cpr % 5 == 0:
                uu, rr = 5, 2
            elif cpr % 3 == 0:
                uu, rr = (3, 4) if M == 1 else (3, 2)
            else:
                uu, rr = 4, 2
            add(tag + " head screen", "_Z23gemv_head_screen_kernelILi%dELi%dELi%dEE" % (M, uu, rr), "screen")
            add(tag + " head re-score", "_Z19head_rescore_kernelILi%dELi%dEE" % (M, 4 if h <= 2048 else 2), "rescore")
    # launch_attention, S == 1, bf16: unsplit -> <bf16,8> (<bf16,4> above 256 (row, head) pairs: not at B <= 2);
    # split with the merge deferred to the dense prologue (B <= 2, linear_parts_supported) -> <bf16,8,32>;
    # split with the ticket merge (the deferral switched off or unsupported) -> <bf16,4>
    add("attention, unsplit", "_Z18attn_decode_kernelIDF16bLi8ELi64EE", "attn")
    add("attention, split, deferred merge", "_Z18attn_decode_kernelIDF16bLi8ELi32EE", "attn")
    add("attention, split, ticket merge", "_Z18attn_decode_kernelIDF16bLi4ELi64EE", "attn")
    return out


# ---- assembly ----
def compile_asm(path):
    from distributed_inference_demo_amd import build as b
    cmd = [b.HIPCC] + b.CFLAGS + ["-S", "--cuda-device-only", os.path.join(b.CSRC, "kernels.hip"), "-o", path]
    print("compiling:", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def split_kernels(text):
    """-> {symbol: [instruction lines]}, {symbol: {amdhsa key: value}}"""
    bodies, meta = {}, {}
    cur = None
    mk = None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            mk = s.split()[1]
            meta[mk] = {}
            continue
        if s == ".end_amdhsa_kernel":
            mk = None
            continue
        if mk is not None and s.startswith(".amdhsa_"):
            p = s.split()
            if len(p) == 2:
                meta[mk][p[0][8:]] = p[1]
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                cur = None
            elif s and not s.startswith((";", ".")) or re.match(r"^\.LBB\w+:", s):
                bodies[cur].append(s.split(";")[0].strip())
    return bodies, meta


SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def sregs(op):
    r = set()
    for a, lo, hi in SREG.findall(op):
        if a:
            r.add(int(a))
        else:
            r.update(range(int(lo), int(hi) + 1))
    return r


def wait_counts(ins):
    vm = re.search(r"vmcnt\((\d+)\)", ins)
    lg = re.search(r"lgkmcnt\((\d+)\)", ins)
    if "vmcnt" not in ins and "lgkmcnt" not in ins and "expcnt" not in ins:  # raw immediate
        m = re.search(r"s_waitcnt\s+(0x[0-9a-f]+|\d+)", ins)
        if m:
            v = int(m.group(1), 0)
            return (v & 0xF) | ((v >> 14) & 0x3) << 4, (v >> 8) & 0xF
    return (int(vm.group(1)) if vm else None), (int(lg.group(1)) if lg else None)


def analyse(body, kind, strict, prologue=False, count_waits=True):
    """-> (listing lines, failures)"""
    listing, fails = [], []
    tainted = set()        # SGPRs holding loaded data (or computed from it)
    s_pending = False      # scalar loads in flight
    karg_waits = 0
    vloads = []            # outstanding vector loads, oldest first: 'kv' / 'w' / 'other'
    barrier_seen = False
    chunk_issued = 0
    chunk_touched = False
    done = False
    issued = False         # gemv: the first weight load went out
    for ins in body:
        if done:
            break
        if ins.endswith(":"):
            continue
        op = ins.split()[0]
        args = ins[len(op):]
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            parts = [a.strip() for a in args.split(",")]
            dst, base = sregs(parts[0]), sregs(parts[1])
            if issued:
                tainted |= dst
                continue
            via = bool(base & tainted)
            listing.append("    %s%s" % (ins, "      <-- through a loaded pointer" if via else ""))
            if via:
                fails.append("scalar load through a loaded pointer: " + ins)
            tainted |= dst
            s_pending = True
            continue
        if op == "s_waitcnt":
            vm, lg = wait_counts(ins)
            note = []
            if lg is not None and s_pending and not issued:
                s_pending = False
                karg_waits += 1
                note.append("scalar wait #%d" % karg_waits)
            if vm is not None and len(vloads) > vm:
                retired = vloads[:len(vloads) - vm]
                vloads = vloads[len(vloads) - vm:]
                note.append("retires %d vector load(s)" % len(retired))
                if kind == "attn":
                    if "kv" in retired:
                        if not barrier_seen:
                            fails.append("K/V loads of the first chunk retired before q is staged: " + ins)
                        chunk_touched = True
                elif issued:  # the first wait behind the weight issue: the prologue's loads, not the weights
                    if prologue and "w" in retired:
                        fails.append("the first wait behind the weight issue retires weight loads: " + ins)
                    done = True
                else:
                    fails.append("vector wait before the first weight load: " + ins)
            if note:
                listing.append("    %-40s ; %s" % (ins, ", ".join(note)))
            if kind == "attn" and chunk_touched:
                done = True
            continue
        if op == "s_barrier":
            listing.append("    s_barrier")
            if kind == "attn":
                barrier_seen = True
            elif issued:
                done = True
            else:
                fails.append("barrier before the first weight load")
            continue
        if op.startswith(("global_load", "buffer_load", "flat_load")):
            if kind == "attn":
                is_kv = "dwordx4" in op
                if barrier_seen:
                    listing.append("    %s" % ins)
                    fails.append("load issued between the q barrier and the first chunk's math: " + ins)
                elif is_kv:
                    chunk_issued += 1
                    if chunk_issued == 1:
                        listing.append("    %s   <-- first K/V load of the chunk" % ins)
                else:
                    if chunk_issued:
                        listing.append("    (%d K/V loads)" % chunk_issued)
                    listing.append("    %s" % ins)
                vloads.append("kv" if is_kv else "other")
            else:
                is_w = " nt" in ins and ("dwordx4" in op or "dwordx2" in op)
                if not issued:
                    listing.append("    %s%s" % (ins, "   <-- first weight load" if is_w else ""))
                vloads.append("w" if is_w else "other")
                if is_w and not issued:
                    issued = True
                    if not prologue:
                        done = True
            continue
        if op.startswith("s_") and not op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_bitcmp", "s_nop",
                                                       "s_sleep", "s_endpgm", "s_setprio", "s_setreg")):
            parts = [a.strip() for a in args.split(",")]
            if len(parts) >= 2:
                dst = sregs(parts[0])
                src = set()
                for p in parts[1:]:
                    src |= sregs(p)
                if src & tainted:
                    tainted |= dst
                else:
                    tainted -= dst
            continue
        if op.startswith("v_readfirstlane") or op.startswith("v_readlane"):
            tainted |= sregs(args.split(",")[0])  # a value that came through a vector register: data
    if kind == "attn":
        listing.insert(0, "    first chunk: %d K/V load instructions" % chunk_issued)
        if not chunk_touched:
            fails.append("scan ended before the first chunk was consumed")
    else:
        allowed = 1 if strict else 2
        if not count_waits:
            listing.append("    (%d scalar waits before the first weight load: reported, not judged)" % karg_waits)
        elif karg_waits > allowed:
            fails.append("%d scalar waits before the first weight load (allowed: %d)" % (karg_waits, allowed))
        elif karg_waits == 2:
            listing.append("    (note: two groups of kernel-argument loads)")
        if not issued:
            fails.append("no weight load found")
    return listing, fails


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--keep")
    ap.add_argument("--strict", action="store_true")
    a = ap.parse_args()
    path = a.asm
    tmp = None
    if not path:
        if a.keep:
            path = a.keep
        else:
            tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
            tmp.close()
            path = tmp.name
        compile_asm(path)
    with open(path) as f:
        bodies, meta = split_kernels(f.read())
    if tmp:
        os.unlink(path)
    bad = 0
    table = []
    for (prefix, kind), labels in decode_instances().items():
        names = [n for n in bodies if n.startswith(prefix)]
        print("== %s" % prefix)
        print("   used by: " + "; ".join(labels))
        if len(names) != 1:
            print("   FAIL: %d symbols match" % len(names))
            bad += 1
            continue
        name = names[0]
        md = meta.get(name, {})
        table.append((prefix, md.get("next_free_vgpr", "?"), md.get("next_free_sgpr", "?"),
                      md.get("private_segment_fixed_size", "?")))
        if kind == "attn":
            listing, fails = analyse(bodies[name], "attn", a.strict)
        else:  # the LayerNorm / embedding prologues: judged past the weight issue too
            m = re.match(r"_Z16gemv_rows_kernelILi\d+ELi\d+ELi\d+ELi(\d+)E", prefix)
            listing, fails = analyse(bodies[name], "gemv", a.strict, prologue=bool(m) and m.group(1) in ("1", "3"),
                                     count_waits=kind != "screen")
        print("\n".join(listing))
        if kind == "rescore":
            print("   (no verdict: count[] / list[] are data dependencies of the candidate tiles)")
        elif fails:
            bad += 1
            for f in fails:
                print("   FAIL: " + f)
        else:
            print("   ok")
    print("\n== registers (.amdhsa metadata): instance, VGPRs, SGPRs, scratch bytes")
    for row in table:
        print("   %-64s %4s %4s %4s" % row)
    print("\n%s: %d instance(s) failed" % ("FAIL" if bad else "PASS", bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
