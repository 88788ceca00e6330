"""Model of the beam mode's parent-word hand-off (csrc/decoder_persist.hip, decoder_persist_beam; DESIGN.md sections 4.4 and 16),
explored over EVERY interleaving of the workgroups of one batch tile (tiles share no wait).

Chain per decoder step s: layer-0 cell -> top-layer cell -> att -> ctx -> log -> CE.  The CE role (P6) writes the parent word of
step s -- which row's state every row continues at step s+1 -- and then makes its PH_CE arrival of step s.  At step s > 0 a cell
reads the parent word of step s-1 to gather h and c:
  the layer-0 cell behind its wait for PH_CE(s-1), the wait the greedy modes already have (the fed token);
  the top-layer cell, whose recurrent half runs early and waits for no P6 in the other modes, behind a wait for PH_CE(s-1) that
  only this mode has.
With one decoder layer there is no top role and att waits for the layer-0 cell.

Checks:
  unwritten_parent   a cell read the parent word of a step whose P6 had not written it;
  deadlock           at a state where no process can move, some process has steps left.
Mutations: `top_no_wait` (the top-layer cell reads the word without its wait), `late_parent` (P6 writes the word behind its arrival)."""


def _program(role, s, layers, top_no_wait, late_parent):
    """Instructions of `role` at step s: ("wait", counter role, counter >= s + offset) | ("pub", role) | ("read",) | ("write",)."""
    if role == "cell":
        return ([("wait", "ce", 0), ("read",), ("wait", "ctx", 0)] if s > 0 else []) + [("pub", "cell")]
    if role == "top":
        head = ([] if top_no_wait else [("wait", "ce", 0)]) + [("read",)] if s > 0 else []
        return head + [("wait", "cell", 1), ("pub", "top")]
    if role == "ce":
        return [("wait", "log", 1)] + ([("pub", "ce"), ("write",)] if late_parent else [("write",), ("pub", "ce")])
    src = {"att": "top" if layers > 1 else "cell", "ctx": "att", "log": "ctx"}[role]
    return [("wait", src, 1), ("pub", role)]


def explore(steps=3, layers=3, top_no_wait=False, late_parent=False):
    """Returns (violations, states explored)."""
    roles = ("cell",) + (("top",) if layers > 1 else ()) + ("att", "ctx", "log", "ce")
    procs0 = tuple((role, 0, 0) for role in roles)          # (role, step, instruction)
    shared0 = (tuple(0 for _ in roles), frozenset())        # (counters, steps whose parent word is written)
    violations, seen, stack = set(), set(), [(procs0, shared0)]
    while stack:
        procs, sh = stack.pop()
        if (procs, sh) in seen:
            continue
        seen.add((procs, sh))
        ctr, written = sh
        moved = False
        for k, (role, s, i) in enumerate(procs):
            if s >= steps:
                continue
            prog = _program(role, s, layers, top_no_wait, late_parent)
            ins = prog[i]
            nsh = sh
            if ins[0] == "wait":
                if ctr[roles.index(ins[1])] < s + ins[2]:
                    continue
            elif ins[0] == "pub":
                c = list(ctr)
                c[roles.index(ins[1])] += 1
                nsh = (tuple(c), written)
            elif ins[0] == "read":
                if s - 1 not in written:
                    violations.add("unwritten_parent")
            elif ins[0] == "write":
                nsh = (ctr, written | {s})
            moved = True
            nxt = (role, s, i + 1) if i + 1 < len(prog) else (role, s + 1, 0)
            stack.append((procs[:k] + (nxt,) + procs[k + 1:], nsh))
        if not moved and any(s < steps for _, s, _ in procs):
            violations.add("deadlock")
    return violations, len(seen)
