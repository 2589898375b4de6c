"""Condition models of stage 2 (reference enhancing/modules/cond/dummycond.py:19-33,72-84): a class label is its own code, so every method is the
identity.  `to_img` (a PIL text rendering for the image logger) and TextCond are left out."""
import os
from typing import Any, List, Tuple, Union

import torch.nn as nn


class DummyCond(nn.Module):
    def __init__(self) -> None:
        super().__init__()

    def encode(self, condition: Any) -> Tuple[Any, Any, Any]:
        return condition, None, condition

    def decode(self, condition: Any) -> Any:
        return condition

    def encode_codes(self, condition: Any) -> Any:
        return condition

    def decode_codes(self, condition: Any) -> Any:
        return condition


class ClassCond(DummyCond):
    def __init__(self, image_size: Union[Tuple[int, int], int], class_name: Union[str, List[str]]) -> None:
        super().__init__()
        self.img_size = image_size
        if isinstance(class_name, str):
            if class_name.endswith("txt") and os.path.isfile(class_name):
                self.cls_name = open(class_name, "r").read().split("\n")
            else:      # a name, or a class file that is not on this machine: kept as given (the names only label logged images)
                self.cls_name = class_name
        elif isinstance(class_name, (list, tuple)) and len(class_name) and isinstance(class_name[0], str):
            self.cls_name = list(class_name)
        else:
            raise Exception("Class file format not supported")
