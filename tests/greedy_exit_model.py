"""Model of the greedy decode's exit protocol (csrc/decoder_persist.hip, decoder_persist_fwd<.., GR = true>),
explored over EVERY interleaving of its workgroups.

Reduced chain per batch tile and decoder step s: cell (waits for its tile's CE of step s-1 -- and reads the stop word behind it -- and
for ctx of s-1) -> att -> ctx -> log -> CE.  The CE role writes the tile's token of step s; when the last row of its tile has emitted
EOS it reports: an atomic max of s into one word, then an arrival on a count of reporting tiles; the tile whose arrival completes the
count writes the stop word n_steps = max + 1, then makes its PH_CE arrival of step s.  A wait made for step s whose counter is not
(yet) satisfied leaves the process once the stop word shows s >= n_steps.

Checks, at every state where no process can move:
  deadlock      every process has finished its steps or left;
  n_steps       the stop word is the first step count at which every row is done (stop_limit if that never happens);
  tokens        every token below n_steps was written;
  early_exit    no process left at a step below n_steps;
  overrun       the tile that wrote the stop word started no step at or past n_steps (its cells read the word behind the arrival).
Mutations: `late_stop` (the stop word written after the PH_CE arrival), `no_check` = role whose wait lacks the stop check."""

ROLES = ("cell", "att", "ctx", "log", "ce")


def _program(role, s, late_stop):
    """Instructions of `role` at step s: ("wait", counter role, counter >= s + offset, recheck) | ("pub", role) | CE actions."""
    if role == "cell":
        return ([("wait", "ce", 0, True), ("wait", "ctx", 0, False)] if s > 0 else []) + [("pub", "cell")]
    if role == "ce":
        tail = [("pub", "ce"), ("stop",)] if late_stop else [("stop",), ("pub", "ce")]
        return [("wait", "log", 1, False), ("token",), ("max",), ("arrive",)] + tail
    src = {"att": "cell", "ctx": "att", "log": "ctx"}[role]
    return [("wait", src, 1, False), ("pub", role)]


def explore(eos_steps, stop_limit=4, late_stop=False, no_check=None):
    """eos_steps: per tile, per row, the step at which the row's argmax is EOS (None: never).  Returns (violations, states explored)."""
    n_tiles = len(eos_steps)
    procs0 = tuple((role, t, 0, 0, "run", -1, False, False, False) for t in range(n_tiles) for role in ROLES)
    # process: (role, tile, step, instruction, status, exit step, reported (CE: max done), arrived (CE), last arriver (CE))
    shared0 = (tuple(0 for _ in range(n_tiles * len(ROLES))), stop_limit, 0, 0, frozenset(), -1)
    # shared: (counters, stop word, max word, arrivals, tokens written, tile that wrote the stop word)

    def tile_done(t, s):
        return all(e is not None and e <= s for e in eos_steps[t])

    def step_proc(p, sh):
        """-> the successor (process, shared), or None when the process cannot move."""
        role, t, s, i, status, xs, rep, arrived, last = p
        ctr, stop, gmax, arr, toks, stopper = sh
        if status != "run":
            return None
        prog = _program(role, s, late_stop)
        ins = prog[i]
        # the next instruction, across the step boundary at once (no separate move for it: fewer interleavings of nothing)
        nxt = (role, t, s, i + 1, status, xs, rep, arrived, last) if i + 1 < len(prog) else \
            (role, t, s + 1, 0, "run" if s + 1 < stop_limit else "done", xs, rep, arrived, last)
        check = role != no_check
        if ins[0] == "wait":
            ok = ctr[ROLES.index(ins[1]) * n_tiles + t] >= s + ins[2]
            if ok and not (ins[3] and check and s >= stop):
                return nxt, sh
            if check and s >= stop:
                return (role, t, s, i, "exit", s, rep, arrived, last), sh
            return None
        if ins[0] == "pub":
            c = list(ctr)
            c[ROLES.index(ins[1]) * n_tiles + t] += 1
            return nxt, (tuple(c), stop, gmax, arr, toks, stopper)
        if ins[0] == "token":
            return nxt, (ctr, stop, gmax, arr, toks | {(t, s)}, stopper)
        if ins[0] == "max":
            if rep or not tile_done(t, s):
                return nxt, sh
            return nxt[:6] + (True, arrived, last), (ctr, stop, max(gmax, s), arr, toks, stopper)
        if ins[0] == "arrive":
            if not rep or arrived:          # (not done yet, or arrived at an earlier step)
                return nxt, sh
            return nxt[:7] + (True, arr + 1 == n_tiles), (ctr, stop, gmax, arr + 1, toks, stopper)
        if ins[0] == "stop":
            if not last or stopper >= 0:
                return nxt, sh
            return nxt, (ctr, gmax + 1, gmax, arr, toks, t)
        raise AssertionError(ins)

    finish = [max(e) if all(x is not None for x in e) and max(e) < stop_limit else None for e in eos_steps]
    expected = max(finish) + 1 if all(f is not None for f in finish) else stop_limit
    violations = set()
    seen = set()
    stack = [(procs0, shared0)]
    while stack:
        procs, sh = stack.pop()
        if (procs, sh) in seen:
            continue
        seen.add((procs, sh))
        moved = False
        for k, p in enumerate(procs):
            r = step_proc(p, sh)
            if r is None:
                continue
            moved = True
            np_, nsh = r
            stack.append((procs[:k] + (np_,) + procs[k + 1:], nsh))
        if moved:
            continue
        ctr, stop, gmax, arr, toks, stopper = sh
        if any(p[4] == "run" for p in procs):
            violations.add("deadlock")
        if stop != expected:
            violations.add("n_steps")
        if any((t, s) not in toks for t in range(n_tiles) for s in range(stop)):
            violations.add("tokens")
        if any(p[4] == "exit" and p[5] < stop for p in procs):
            violations.add("early_exit")
        if stopper >= 0 and ctr[ROLES.index("cell") * n_tiles + stopper] > stop:
            violations.add("overrun")
    return violations, len(seen)
