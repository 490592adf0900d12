"""``InstanceDuplicator`` under the reference's name (data/instance_duplicator.py): a clip with a lone instance gets a shifted,
optionally mirrored copy of it pasted into every frame.  The reference decides and applies in one go with numpy and cv2.warpAffine; here
the DECISION is made on the host from the annotation strings alone -- boxes by an integer walk over the RLE runs, then the reference's
logic line for line, its calls to ``random.random()`` in its order and number -- and ``hip.duplicate_instance`` applies it on the
device.  cv2 quantises the shift to 1/32 pixel; the device kernel does not."""
import random

import numpy as np



def string_to_counts(s):
    """pycocotools' rleFrString: characters - 48 in 5-bit groups, least significant first, 0x20 = more follows, the sign from bit 0x10 of
    the last group; counts from the fourth on are deltas against the count two places earlier.  (The same walk as
    inference/output_utils/coco_rle.py, restated here because nothing a DataLoader worker imports may load the HIP binding.)"""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_area_and_box(rle, height, width):
    """A COCO RLE string (column-major runs, the first counting zeros) -> (area, box): the number of set pixels and the reference's
    ``bbox_from_mask`` -- (xmin, ymin, xmax, ymax) with EXCLUSIVE maxima, or None for an empty mask -- in integers, without decoding."""
    counts = [int(c) for c in string_to_counts(rle.decode("latin-1") if isinstance(rle, (bytes, bytearray)) else rle)]
    if sum(counts) != height * width or any(c < 0 for c in counts):
        raise ValueError("the annotation is no valid COCO RLE for a %d x %d mask" % (height, width))
    area, pos = 0, 0
    xmin, ymin, xmax, ymax = width, height, 0, 0
    for j, c in enumerate(counts):
        if j % 2 == 1 and c > 0:
            first, last = pos, pos + c - 1
            x0, x1 = first // height, last // height
            y0, y1 = (first % height, last % height) if x0 == x1 else (0, height - 1)          # a run over a column boundary spans the height
            xmin, xmax, ymin, ymax = min(xmin, x0), max(xmax, x1 + 1), min(ymin, y0), max(ymax, y1 + 1)
            area += c
        pos += c
    return area, (None if area == 0 else (xmin, ymin, xmax, ymax))


class InstanceDuplicator(object):
    def __call__(self, boxes, width, height):
        """boxes: per frame (xmin, ymin, xmax, ymax) with exclusive maxima, or None -> {"flip": bool, "shifts": [(shift_x, shift_y) | None
        per frame]}, or None where the reference gives up (an infeasible case, or any exception): the sample then stays as it is."""
        try:
            return self._decide(boxes, width, height)
        except Exception as err:          # (the reference: "lots of potentially unstable stuff happening here")
            print("Exception occurred trying to duplicate instance")
            print(err)
            return None

    @staticmethod
    def _decide(boxes, mask_width, mask_height):
        horiz_multiplier = None
        vert_multiplier = None
        touches_left_boundary, touches_right_boundary = False, False
        touches_top_boundary, touches_bottom_boundary = False, False

        for bbox in boxes:
            if bbox is None:
                continue
            xmin, ymin, xmax, ymax = bbox

            if xmin == 0:
                touches_left_boundary = True
            if xmax == mask_width:
                touches_right_boundary = True
            if ymin == 0:
                touches_top_boundary = True
            if ymax == mask_height:
                touches_bottom_boundary = True

            if xmax - xmin > 0.4 * mask_width:            # wide: only further out of the frame on the side it touches
                if xmin == 0:
                    horiz_multiplier = -1.
                elif xmax == mask_width:
                    horiz_multiplier = 1.
            elif xmax - xmin < 0.2 * mask_width:          # narrow and near a side: only away from it
                xc = (xmin + xmax) / 2.
                if xc < mask_width * 0.25:
                    horiz_multiplier = 1.
                elif xc > mask_width * 0.75:
                    horiz_multiplier = -1.

            if ymax - ymin > 0.4 * mask_height:
                if ymin == 0:
                    vert_multiplier = -1.
                elif ymax == mask_height:
                    vert_multiplier = 1.
            elif ymax - ymin < 0.2 * mask_height:
                yc = (ymin + ymax) / 2.
                if yc < mask_height * 0.25:
                    vert_multiplier = 1.
                elif yc > mask_height * 0.75:
                    vert_multiplier = -1.

        if touches_left_boundary and touches_right_boundary:
            return None
        flipping_feasible = (not touches_left_boundary) and (not touches_right_boundary)
        if touches_bottom_boundary and touches_top_boundary:
            vert_multiplier = 0.
        if horiz_multiplier is None:
            horiz_multiplier = -1 if random.random() < 0.5 else 1.
        if vert_multiplier is None:
            vert_multiplier = -1 if random.random() < 0.5 else 1.
        flip = random.random() < 0.5 if flipping_feasible else False

        shifts = []
        for bbox in boxes:
            if bbox is None:
                shifts.append(None)
                continue
            xmin, ymin, xmax, ymax = bbox
            width, height = xmax - xmin, ymax - ymin
            shift_x = horiz_multiplier * ((width * 0.75) + (random.random() * 0.25 * width))
            shift_y = vert_multiplier * (height * random.random() * 0.25)
            shift_x = min(shift_x, mask_width * 0.3)
            shift_y = min(shift_y, mask_height * 0.3)
            shifts.append((float(np.float32(shift_x)), float(np.float32(shift_y))))          # the reference's matrix is float32
        return {"flip": bool(flip), "shifts": shifts}
