"""The NumPy twin of the library's limited-memory Hessian (include/asm_hip.h, "Limited-memory Hessian"): a limited-memory BFGS
approximation B of the Hessian of L = f - lambda' g in the compact form of Byrd, Nocedal and Schnabel over the stored pairs in
chronological order,

    B v = sigma v - Psi' W Psi v,   Psi = [sigma S; Y],   W = [[sigma S S', L], [L', -D]]^-1,

sigma = y'y / s'y of the newest pair, D = diag(s_i'y_i), L_ij = s_i'y_j for i > j.  No pairs: B = I.  A pair is stored only if
||s|| > 0, s'y > 0 and s'y >= 1e-8 ||s|| ||y||; a push to a full store drops the oldest pair.

    LMHessian.push_pair(s, y)              offer a pair (True: stored)
    LMHessian.begin(x, grad_lag) / end     the pair of a step: s = x_end - x_begin, y = grad_lag_end - grad_lag_begin, grad_lag the
                                           gradient of the Lagrangian at the two points with the same multipliers
    LMHessian.product(V)                   B v, or the rows of V [k x n] times B, through W as the device forms it (block elimination
                                           with a Cholesky factor of sigma S S' + L D^-1 L')
    LMHessian.dense()                      B by the textbook recursive BFGS update from sigma I: an independent route to the same matrix
    LMHessian.info()                       memory, pairs, pushed, skipped_zero, skipped_curvature, sigma
"""
import numpy as np

LM_MAX = 32
CURVATURE = 1e-8               # a pair is stored only if s'y >= CURVATURE ||s|| ||y||


class LMHessian:
    def __init__(self, n, memory=10):
        if not 1 <= int(memory) <= LM_MAX:
            raise ValueError("memory = %r: expected 1 .. %d" % (memory, LM_MAX))
        self.n, self.memory = int(n), int(memory)
        self.reset()

    def reset(self):
        self.S, self.Y = np.zeros((0, self.n)), np.zeros((0, self.n))      # chronological, oldest first
        self.sigma = 1.0
        self.pushed = self.skipped_zero = self.skipped_curvature = 0
        self._pending = None
        self._W = None

    def push_pair(self, s, y):
        s, y = np.asarray(s, float), np.asarray(y, float)
        if s.shape != (self.n,) or y.shape != (self.n,):
            raise ValueError("s / y have shapes %r / %r, expected (%d,)" % (s.shape, y.shape, self.n))
        self.pushed += 1
        ns, ny, sy = float(np.sqrt(s @ s)), float(np.sqrt(y @ y)), float(s @ y)
        if not ns > 0.0:
            self.skipped_zero += 1
            return False
        if not (sy > 0.0 and sy >= CURVATURE * ns * ny):          # (s'y > 0 too: y = 0 meets the inequality)
            self.skipped_curvature += 1
            return False
        self.S = np.vstack([self.S, s])[-self.memory:]
        self.Y = np.vstack([self.Y, y])[-self.memory:]
        self.sigma = float(y @ y) / sy
        self._W = None
        return True

    def begin(self, x, grad_lag):
        self._pending = (np.array(x, float), np.array(grad_lag, float))

    def end(self, x, grad_lag):
        """The pair since begin(); nothing (None) without a pending begin."""
        if self._pending is None:
            return None
        x0, g0 = self._pending
        self._pending = None
        return self.push_pair(np.asarray(x, float) - x0, np.asarray(grad_lag, float) - g0)

    @property
    def pairs(self):
        return len(self.S)

    def middle(self):
        """W [2p x 2p]: with C = sigma S S' + L D^-1 L' (symmetric positive definite), G = C^-1 L D^-1,
        W = [[C^-1, G], [G', D^-1 L' G - D^-1]]."""
        if self._W is None:
            p = self.pairs
            SY = self.S @ self.Y.T
            L, dinv = np.tril(SY, -1), 1.0 / np.diag(SY)
            C = self.sigma * (self.S @ self.S.T) + (L * dinv) @ L.T
            R = np.linalg.cholesky(C)
            Ci = np.linalg.solve(R.T, np.linalg.solve(R, np.eye(p)))
            G = (Ci @ L) * dinv
            self._W = np.block([[Ci, G], [G.T, dinv[:, None] * (L.T @ G) - np.diag(dinv)]])
        return self._W

    def product(self, V):
        V = np.asarray(V, float)
        if V.shape[-1:] != (self.n,) or V.ndim not in (1, 2):
            raise ValueError("V has shape %r, expected (%d,) or (k, %d)" % (V.shape, self.n, self.n))
        if not self.pairs:
            return V.copy()
        Psi = np.vstack([self.sigma * self.S, self.Y])
        return self.sigma * V - ((V @ Psi.T) @ self.middle()) @ Psi

    def dense(self):
        """B_0 = sigma I, then B <- B - (B s)(B s)' / (s' B s) + y y' / (s'y) over the stored pairs, oldest first."""
        B = self.sigma * np.eye(self.n)
        for s, y in zip(self.S, self.Y):
            Bs = B @ s
            B = B - np.outer(Bs, Bs) / float(s @ Bs) + np.outer(y, y) / float(s @ y)
        return B

    def info(self):
        return dict(memory=self.memory, pairs=self.pairs, pushed=self.pushed, skipped_zero=self.skipped_zero,
                    skipped_curvature=self.skipped_curvature, sigma=self.sigma)
