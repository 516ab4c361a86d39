"""Float64 reference of Block.lstm_aggregate (tests only): the step loop of include/coala_hip.h's contract in numpy, row by row, with
both gradients by hand (no autograd)."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def valid_rows(nbr):
    """The valid sources of every row of a -1 padded [n_dst, fanout] array, in slot order."""
    return [[int(s) for s in row if s >= 0] for row in nbr]


def lstm_ref(rows, xg, w_hh, grad_out):
    """rows: per destination the list of its sources in slot order -> (out [n_dst, H], grad_xg, grad_w_hh), float64."""
    xg, w, go = xg.astype(np.float64), w_hh.astype(np.float64), grad_out.astype(np.float64)
    H = w.shape[1]
    out, gx, gw = np.zeros((len(rows), H)), np.zeros(xg.shape), np.zeros(w.shape)
    for d, srcs in enumerate(rows):
        h, c, tape = np.zeros(H), np.zeros(H), []
        for s in srcs:
            z = xg[s] + w @ h
            i, f, g, o = _sig(z[:H]), _sig(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), _sig(z[3 * H:])
            c_new = f * c + i * g
            tape.append((s, h, c, i, f, g, o, np.tanh(c_new)))
            h, c = o * np.tanh(c_new), c_new
        out[d] = h
        dh, dc = go[d], np.zeros(H)
        for s, h_prev, c_prev, i, f, g, o, tc in reversed(tape):
            dc = dc + dh * o * (1 - tc * tc)
            dz = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)])
            gx[s] += dz
            gw += np.outer(dz, h_prev)
            dh, dc = w.T @ dz, dc * f
    return out, gx, gw
