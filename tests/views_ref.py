"""Plain-numpy reference of the pooled-view detect (DESIGN.md section 3 "Pooled views"; csrc/detect_wide.hip ``detect_views_select_kernel``).
No torch.

``map_boxes``: a view's canvas boxes in image coordinates, fp32 op for op -- ``x / sx + dx``, ``y / sy + dy`` (one division, one
addition), then for a flipped view ``(x1, x2) <- (mirror - x2, mirror - x1)``.
``pooled_filter``: the mapped candidates of an image's V views concatenated in view order, then ``nms_ref.soft_filter`` on them; the
pooled index of a row is its index into that concatenation, ``v * A + anchor``."""
import numpy as np

import nms_ref

F = np.float32
IDENTITY = np.array([1, 1, 0, 0, 0, 0], F)


def map_boxes(boxes, xf):
    """boxes [n, 4] xyxy on a view's canvas, xf [6] = (sy, sx, dy, dx, flip, mirror) -> fp32 [n, 4] in image coordinates."""
    b = np.asarray(boxes, F).reshape(-1, 4)
    sy, sx, dy, dx, flip, mirror = (F(v) for v in np.asarray(xf, F).reshape(6))
    out = np.empty_like(b)
    out[:, 0] = (b[:, 0] / sx).astype(F) + dx
    out[:, 1] = (b[:, 1] / sy).astype(F) + dy
    out[:, 2] = (b[:, 2] / sx).astype(F) + dx
    out[:, 3] = (b[:, 3] / sy).astype(F) + dy
    if flip != 0:
        x1 = mirror - out[:, 2]
        x2 = mirror - out[:, 0]
        out[:, 0], out[:, 2] = x1, x2
    return out.astype(F)


def pool(class_ids, scores, boxes, xf):
    """Per-view dense tensors of ONE image ([V, A], [V, A], [V, A, 4]) and its xf [V, 6] -> the pooled ([V*A], [V*A], [V*A, 4])."""
    class_ids, scores = np.asarray(class_ids), np.asarray(scores, F)
    boxes = np.asarray(boxes, F)
    V = scores.shape[0]
    mapped = np.concatenate([map_boxes(boxes[v], xf[v]) for v in range(V)], 0)
    return class_ids.reshape(-1), scores.reshape(-1), mapped


def pooled_filter(class_ids, scores, boxes, xf, K, nms_thresh, score_thresh, num_classes, mode='hard', sigma=0.5, agnostic=False):
    """``nms_ref.soft_filter`` on the pooled candidates of one image; ``anchor_idx`` of the result is the pooled index."""
    c, s, b = pool(class_ids, scores, boxes, xf)
    return nms_ref.soft_filter(c, s, b, K, nms_thresh, score_thresh, num_classes, mode, sigma, agnostic)
