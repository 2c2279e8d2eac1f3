"""NumPy restatement of the device-resident L-BFGS loop, written from its specification (include/qoc.h, qoc_lbfgs_params), not from the kernel:
the plain two-loop recursion on explicit vectors, backtracking Armijo, state fields and flags as the specification names them.

    st = LbfgsState(params)
    x = st.step(x, f, g, loss, g2)        # one evaluation's decision; st.done ends the run, st.branch names what happened

`run(evaluate, x0, params, n)` drives it with a callable x -> dict(reg_loss, grad, loss, grad_squared) and records every evaluation.
"""
import numpy as np

DEFAULTS = dict(conv_target=1e-8, min_grad=1e-25, c1=1e-4, shrink=0.5, max_iterations=5000, history=8, max_ls=20)

# what one evaluation led to
ACCEPT, REJECT, RESET, STALL, RESTORE, STOP = 'accept', 'reject', 'reset', 'stall', 'restore', 'stop'


class LbfgsState(object):
    def __init__(self, params=None):
        p = dict(DEFAULTS)
        p.update(params or {})
        self.p = p
        self.x_acc = self.g_acc = self.p_dir = None
        self.f_acc = 0.0
        self.alpha = 0.0
        self.gp = 0.0
        self.ls = 0
        self.S, self.Y = [], []            # oldest first
        self.first = True
        self.restoring = False
        self.done = False
        self.iters = 0
        # records of the last step
        self.branch = None
        self.margin = None                 # f - (f_acc + c1 alpha gp); None on the first evaluation
        self.curvature = None              # (sy - 1e-10 yy) of an accepted step past the first
        self.pushed = None
        self.cleared = False               # the accept found g.p >= 0 and fell back to steepest descent

    def _direction(self, g):
        """-H g by the two-loop recursion, H0 = (sy / yy) I of the newest pair; -g / |g| with an empty history or when the result is no descent direction."""
        self.cleared = False
        if self.S:
            q = g.copy()
            a = [0.0] * len(self.S)
            for i in range(len(self.S) - 1, -1, -1):
                a[i] = np.dot(self.S[i], q) / np.dot(self.S[i], self.Y[i])
                q = q - a[i] * self.Y[i]
            r = (np.dot(self.S[-1], self.Y[-1]) / np.dot(self.Y[-1], self.Y[-1])) * q
            for i in range(len(self.S)):
                beta = np.dot(self.Y[i], r) / np.dot(self.S[i], self.Y[i])
                r = r + self.S[i] * (a[i] - beta)
            p = -r
            if np.dot(g, p) >= 0:
                self.S, self.Y = [], []
                self.cleared = True
                p = -(g / np.linalg.norm(g))
        else:
            p = -(g / np.linalg.norm(g))
        return p

    def step(self, x, f, g, loss, g2):
        """The decision after the evaluation of x (f = reg_loss, g its gradient, loss and g2 = grad_squared for the stop rule); the next point."""
        p = self.p
        x = np.asarray(x, dtype=np.float64)
        g = np.asarray(g, dtype=np.float64)
        self.margin = self.curvature = self.pushed = None
        if self.done:
            self.branch = None
            return x
        if self.restoring:
            self.done, self.branch = True, STOP
            return x
        if loss < p['conv_target'] or g2 < p['min_grad']:
            self.done, self.branch = True, STOP
            return x
        if not self.first:
            self.margin = f - (self.f_acc + p['c1'] * self.alpha * self.gp)
        acceptable = self.first or bool(np.isfinite(f) and f <= self.f_acc + p['c1'] * self.alpha * self.gp)
        if self.iters >= p['max_iterations']:
            if acceptable:
                self.done, self.branch = True, STOP
                return x
            self.restoring, self.branch = True, RESTORE
            return self.x_acc.copy()
        self.iters += 1
        if acceptable:
            if not self.first:
                s, y = x - self.x_acc, g - self.g_acc
                sy, yy = np.dot(s, y), np.dot(y, y)
                self.curvature = sy - 1e-10 * yy
                self.pushed = bool(sy > 1e-10 * yy)
                if self.pushed:
                    self.S.append(s)
                    self.Y.append(y)
                    if len(self.S) > p['history']:
                        self.S.pop(0)
                        self.Y.pop(0)
            self.first = False
            self.x_acc, self.g_acc, self.f_acc = x.copy(), g.copy(), float(f)
            self.p_dir = self._direction(g)
            self.gp = float(np.dot(self.g_acc, self.p_dir))
            self.alpha, self.ls = 1.0, 0
            self.branch = ACCEPT
            return self.x_acc + self.p_dir
        self.ls += 1
        self.branch = REJECT
        if self.ls > p['max_ls']:
            if not self.S:
                self.restoring, self.branch = True, STALL
                return self.x_acc.copy()
            self.S, self.Y = [], []
            self.p_dir = -(self.g_acc / np.linalg.norm(self.g_acc))
            self.gp = float(np.dot(self.g_acc, self.p_dir))
            self.alpha = 1.0 / p['shrink']
            self.ls = 0
            self.branch = RESET
        self.alpha *= p['shrink']
        return self.x_acc + self.alpha * self.p_dir


def run(evaluate, x0, params=None, n=None):
    """Drive LbfgsState with `evaluate(x) -> dict(reg_loss, grad, loss, grad_squared)` from x0 for n evaluations (None: until done, at most
    max_iterations + 2).  Returns dict(x: the point after the last step, state, points: the evaluated points, f, loss, branch, margin, curvature,
    pushed, wrapped: the evaluations at which a full history dropped its oldest pair, cleared)."""
    st = LbfgsState(params)
    budget = st.p['max_iterations'] + 2 if n is None else n
    x = np.array(x0, dtype=np.float64)
    shape = x.shape
    rec = dict(points=[], f=[], loss=[], branch=[], margin=[], curvature=[], pushed=[], wrapped=[], cleared=[], next=[])
    for i in range(budget):
        if st.done:
            break
        r = evaluate(x)
        full = len(st.S) == st.p['history']
        rec['points'].append(x.copy())
        rec['f'].append(float(r['reg_loss']))
        rec['loss'].append(float(r['loss']))
        x = st.step(x.reshape(-1), r['reg_loss'], np.asarray(r['grad'], dtype=np.float64).reshape(-1), r['loss'], r['grad_squared']).reshape(shape)
        rec['branch'].append(st.branch)
        rec['margin'].append(st.margin)
        rec['curvature'].append(st.curvature)
        rec['pushed'].append(st.pushed)
        rec['cleared'].append(st.cleared and st.branch == ACCEPT)
        rec['next'].append(x.copy())
        if full and st.pushed:
            rec['wrapped'].append(i)
    rec['x'] = x
    rec['state'] = st
    return rec
